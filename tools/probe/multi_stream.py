#!/usr/bin/env python3
"""The chunks of many connections: one call per connection chunk against one call for all of them.
    tools/probe/multi_stream.py [--window 0.5] [--rounds 3] [--cells K:chunk,K:chunk,...]
Corpus: cfg2-style RFC5424 lines (flowgger_amd/synth.py); a connection's chunk is whole lines up to the chunk size plus the first
half of the next line (so every chunk has an unterminated tail: `consumed` < nbytes on side A, a CARRY slot on side B); pinned host
buffers on all sides; K connections x chunk bytes, the total capped at 256 MiB (K shrinks).
    A    one fg_frame_decode_batch(final = 0) call per connection chunk on one ctx, in sequence (chunks 16-byte aligned in their buffer)
    A8   the same over eight fg_clone'd ctxs on eight threads (connection k on thread k % 8)
    B    ONE fg_frame_decode_multi_batch call (chunks back to back, no alignment)
Per cell: the canonical Record bytes of A's rows and of B's FRAME rows are asserted equal (every connection up to 64 MiB, 64 evenly
spaced ones beyond); then windows of at least --window seconds, the sides alternated within one process, --rounds rounds; median and
spread (min .. max) of lines/s end to end.  Framing alone: device time between two events around fg_frame_multi_device (K segments)
and around fg_frame_device (the same bytes as one stream), both HBM-resident, median of 15 -- what the boundary handling costs.
(fg_set_timing covers the decode launches only, so events around the calls stand in for it.)  One JSON line at the end.
    --transcode  the same cells (--transcode-cells) through the encoder too (GELF + line merger), three sides alternated in one process:
               T    ONE fg_transcode_multi_batch call on side B's pinned buffer
               A-t  one fg_transcode_batch(final = 0) call per connection chunk on side A's pinned buffer
               B    as above: the tables of ONE fg_frame_decode_multi_batch call cross the link
               T's stream is asserted equal to A-t's streams back to back.  Per side: lines/s end to end, median and spread, and the
               bytes that cross the link each way per batch, computed from the sizes the calls return.
    --syslen   octet-counted chunks instead ("<len> <line>\\n" frames, a connection's chunk ends inside a frame), HBM-resident: the time
               between two events around ONE fg_frame_syslen_multi_device call against K fg_frame_syslen_device calls on the same bytes
               (every chunk 16-byte aligned in a buffer of its own; each call synchronises, as it must to return its counts), for
               --syslen-cells K:chunk,...; and one stream (--syslen-one bytes) with n_segs == 1 against the single-stream call -- what
               the segment lookup costs when it finds nothing.  Median (min .. max) of 9 after 3 warm-up runs.
    --capnp    Cap'n Proto chunks instead (single-segment messages of 6 .. 70 words whose bodies hold pointer-like words, zero words
               and text; a connection's chunk ends inside a message, on a word), HBM-resident: ONE fg_frame_capnp_multi_device call
               against K fg_frame_capnp_device calls on the same bytes, for --capnp-cells K:chunk,...; and one stream (--capnp-one bytes)
               with n_segs == 1 against the single-stream call.  Timed as --syslen."""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent.parent))
import torch  # noqa: E402

from flowgger_amd import RFC5424Decoder, synth  # noqa: E402
from flowgger_amd import _lib as L  # noqa: E402
from flowgger_amd.tables import HostTables  # noqa: E402

CAP_TOTAL = 256 << 20
u64p = C.POINTER(C.c_uint64)


def pinned(nbytes):
    p = C.c_void_p()
    L.check(L.lib().fg_alloc_pinned(nbytes + 64, C.byref(p)), "fg_alloc_pinned")
    return p, np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), (nbytes + 64,))


def build_cell(lines, K, chunk):
    """-> (chunks as bytes, lines per chunk); the corpus is walked round and round"""
    out, counts, i = [], [], 0
    for _ in range(K):
        buf, n = bytearray(), 0
        while True:
            ln = lines[i % len(lines)]
            i += 1
            if len(buf) + len(ln) + 1 > chunk:
                buf += ln[: max(1, min(len(ln) // 2, chunk - len(buf)))]  # the unterminated tail
                break
            buf += ln + b"\n"
            n += 1
        out.append(bytes(buf))
        counts.append(n)
    return out, counts


class SideA:
    def __init__(self, dec, chunks):
        self.dec = dec
        self.offs = np.zeros(len(chunks) + 1, np.int64)
        for k, c in enumerate(chunks):
            self.offs[k + 1] = (self.offs[k] + len(c) + 15) & ~15
        self.lens = [len(c) for c in chunks]
        self.p, self.buf = pinned(int(self.offs[-1]) + 16)
        for k, c in enumerate(chunks):
            self.buf[self.offs[k]:self.offs[k] + len(c)] = np.frombuffer(c, np.uint8)

    def one(self, dec, k):
        st, off, n, used = L.fg_tables(), C.c_void_p(), C.c_uint64(), C.c_uint64()
        L.check(L.lib().fg_frame_decode_batch(dec._ctx, dec.fmt, L.FG_FRAME_LINE, self.p.value + int(self.offs[k]), self.lens[k], 0, C.byref(st),
                                              C.byref(off), C.byref(n), C.byref(used)), "fg_frame_decode_batch")
        return st, off, int(n.value)

    def run(self):
        return sum(self.one(self.dec, k)[2] for k in range(len(self.lens)))

    def rows(self, k):
        """canonical bytes of chunk k's rows"""
        st, off, n = self.one(self.dec, k)
        if n == 0:
            return b""
        offsets = np.ctypeslib.as_array(C.cast(off, u64p), (n + 1,)).copy()
        blob, _ = HostTables.from_struct(st).serialize(self.dec.fmt, self.buf[self.offs[k]:], offsets)
        return blob.tobytes()


class SideA8(SideA):
    def __init__(self, dec, a: SideA):
        self.__dict__.update(a.__dict__)
        self.clones = [dec.clone_boxed() for _ in range(8)]
        self.pool = ThreadPoolExecutor(8)

    def run(self):
        K = len(self.lens)
        return sum(self.pool.map(lambda t: sum(self.one(self.clones[t], k)[2] for k in range(t, K, 8)), range(8)))


class SideB:
    def __init__(self, dec, chunks):
        self.dec = dec
        self.starts = np.zeros(len(chunks) + 1, np.uint64)
        self.starts[1:] = np.cumsum([len(c) for c in chunks], dtype=np.uint64)
        self.n = int(self.starts[-1])
        self.p, self.buf = pinned(self.n + 16)
        self.buf[:self.n] = np.frombuffer(b"".join(chunks), np.uint8)
        self.K = len(chunks)

    def call(self):
        st, n = L.fg_tables(), C.c_uint64()
        v = [C.c_void_p() for _ in range(4)]
        L.check(L.lib().fg_frame_decode_multi_batch(self.dec._ctx, self.dec.fmt, L.FG_FRAME_LINE, self.p, self.n, self.starts.ctypes.data, None, self.K,
                                                    C.byref(st), *[C.byref(x) for x in v], C.byref(n)), "fg_frame_decode_multi_batch")
        return st, v, int(n.value)

    def run(self):
        st, v, n = self.call()
        return n - self.K  # (every chunk ends in a CARRY slot)

    def tables(self):
        st, v, n = self.call()
        offsets = np.ctypeslib.as_array(C.cast(v[0], u64p), (n + 1,)).copy()
        kind = np.ctypeslib.as_array(C.cast(v[1], C.POINTER(C.c_uint8)), (n,)).copy()
        first = np.ctypeslib.as_array(C.cast(v[2], u64p), (self.K + 1,)).copy()
        return HostTables.from_struct(st), offsets, kind, first


class SideT:
    """ONE fg_transcode_multi_batch call on side B's pinned buffer"""

    def __init__(self, b: SideB, ecfg):
        self.b, self.ecfg, self.res = b, ecfg, L.fg_transcoded_multi()

    def run(self):
        b = self.b
        L.check(L.lib().fg_transcode_multi_batch(b.dec._ctx, b.dec.fmt, L.FG_FRAME_LINE, C.byref(self.ecfg), b.p, b.n, b.starts.ctypes.data, None, b.K,
                                                 C.byref(self.res)), "fg_transcode_multi_batch")
        return int(self.res.n) - b.K  # (every chunk ends in a CARRY slot)

    def out(self):
        self.run()
        return np.ctypeslib.as_array(C.cast(self.res.out, C.POINTER(C.c_uint8)), (int(self.res.out_bytes),)).tobytes()

    def link_bytes(self):
        """(up, down) of one call, from what it returned: the buffer and the starts; the stream, its offsets, meta and enc_status, and
        the mirror of the per-segment and per-slot lists"""
        n, K = int(self.res.n), self.b.K
        return self.b.n + (K + 1) * 8, int(self.res.out_bytes) + (n + 1) * 8 + 5 * n + (K + 1) * 8 + K * 8 + (n + 1) * 8 + n


class SideAt:
    """one fg_transcode_batch(FG_FRAME_LINE, final = 0) call per connection chunk on side A's pinned buffer"""

    def __init__(self, a: SideA, ecfg):
        self.a, self.ecfg, self.res = a, ecfg, L.fg_transcoded()
        self.up = self.down = 0

    def one(self, k):
        a = self.a
        L.check(L.lib().fg_transcode_batch(a.dec._ctx, a.dec.fmt, L.FG_FRAME_LINE, C.byref(self.ecfg), a.p.value + int(a.offs[k]), a.lens[k], None, 0, 0,
                                           C.byref(self.res)), "fg_transcode_batch")
        n = int(self.res.n)
        self.up += a.lens[k]
        self.down += int(self.res.out_bytes) + 2 * (n + 1) * 8 + 5 * n  # (the stream, out_offsets and frame_offsets, meta and enc_status)
        return n

    def run(self):
        return sum(self.one(k) for k in range(len(self.a.lens)))

    def out(self):
        parts = []
        for k in range(len(self.a.lens)):
            self.one(k)
            parts.append(np.ctypeslib.as_array(C.cast(self.res.out, C.POINTER(C.c_uint8)), (max(int(self.res.out_bytes), 1),))[:int(self.res.out_bytes)].tobytes())
        return b"".join(parts)

    def link_bytes(self):
        self.up = self.down = 0
        self.run()
        return self.up, self.down


def transcode_mode(dec, lines, cells, seconds, rounds):
    """sides T, A-t and B alternated in one process; per side the bytes that cross the link each way, from the sizes the calls return"""
    from flowgger_amd import GelfEncoder

    ecfg, _keep = GelfEncoder(None, merger="line")._cfg_struct(0.0)
    results = []
    for K0, chunk in cells:
        K = max(1, min(K0, CAP_TOTAL // chunk))
        chunks, counts = build_cell(lines, K, chunk)
        a, b = SideA(dec, chunks), SideB(dec, chunks)
        t, at = SideT(b, ecfg), SideAt(a, ecfg)
        assert t.out() == at.out(), "one call and a call per chunk: the streams differ"
        assert t.run() == at.run() == b.run() == sum(counts)
        tab = b.tables()[0]
        nb = int(tab.n)
        link = {"T": t.link_bytes(), "A-t": at.link_bytes(),
                "B": (b.n + (K + 1) * 8, 68 * nb + 18 * int(tab.ent_used) + (K + 1) * 8 + K * 8 + (nb + 1) * 8 + nb)}
        sides = {"T": t.run, "A-t": at.run, "B": b.run}
        for fn in sides.values():  # warm-up: every shape the windows use
            fn(), fn()
        rates, per_call = {s: [] for s in sides}, {}
        for _ in range(rounds):
            for s, fn in sides.items():
                r, dt = window(fn, seconds)
                rates[s].append(r)
                per_call[s] = dt
        row = {"K": K, "K_asked": K0, "chunk": chunk, "bytes": sum(len(c) for c in chunks), "lines": sum(counts)}
        for s in sides:
            row[s] = {"lines_per_s": statistics.median(rates[s]), "min": min(rates[s]), "max": max(rates[s]), "ms_per_batch": per_call[s] * 1e3,
                      "bytes_up": link[s][0], "bytes_down": link[s][1]}
        results.append(row)
        print(f"K={K:5d} chunk={chunk:8d} total={row['bytes'] / 2**20:7.1f} MiB  " +
              "  ".join(f"{s} {row[s]['lines_per_s'] / 1e6:7.2f} M lines/s ({row[s]['min'] / 1e6:.2f}..{row[s]['max'] / 1e6:.2f}; {row[s]['ms_per_batch']:.2f} ms; "
                        f"up {link[s][0] / 2**20:.2f} MiB, down {link[s][1] / 2**20:.2f} MiB)" for s in sides), flush=True)
        L.lib().fg_free_pinned(a.p)
        L.lib().fg_free_pinned(b.p)
    print(json.dumps({"probe": "multi_stream_transcode", "window_s": seconds, "rounds": rounds, "cells": results}))


def window(fn, seconds):
    t0 = time.perf_counter()
    lines = calls = 0
    while True:
        lines += fn()
        calls += 1
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return lines / dt, dt / calls


def frame_only(dec, chunks, dev):
    raw = b"".join(chunks)
    host = np.zeros(((len(raw) + 15) & ~15) + 16, np.uint8)
    host[:len(raw)] = np.frombuffer(raw, np.uint8)
    d_bytes = torch.from_numpy(host).to(dev)[:len(raw)]
    starts = np.zeros(len(chunks) + 1, np.int64)
    starts[1:] = np.cumsum([len(c) for c in chunks])
    d_starts = torch.from_numpy(starts).to(dev)
    s = torch.cuda.current_stream(dev)

    def timed(fn):
        ts = []
        for i in range(18):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            fn()
            b.record(s)
            torch.cuda.synchronize(dev)
            if i >= 3:
                ts.append(a.elapsed_time(b) * 1e3)
        return statistics.median(ts), min(ts), max(ts)

    cap = len(raw) // 32 + len(chunks) + 1024
    multi = timed(lambda: dec.frame_multi_device(d_bytes, d_starts, None, L.FG_FRAME_LINE, cap_slots=cap))
    single = timed(lambda: dec.frame_device(d_bytes, L.FG_FRAME_LINE, cap_frames=cap))
    return multi, single


def syslen_chunks(lines, K, chunk):
    """K chunks of about `chunk` bytes: whole frames, then the first half of the next one"""
    out, i = [], 0
    for _ in range(K):
        buf = bytearray()
        while True:
            ln = lines[i % len(lines)]
            i += 1
            f = b"%d %s\n" % (len(ln) + 1, ln)
            if len(buf) + len(f) > chunk:
                buf += f[:max(1, min(len(f) // 2, chunk - len(buf)))]
                break
            buf += f
        out.append(bytes(buf))
    return out


def syslen_mode(dec, lines, dev, cells, one_bytes):
    def to_dev(raw):
        host = np.zeros(((len(raw) + 15) & ~15) + 16, np.uint8)
        host[:len(raw)] = np.frombuffer(raw, np.uint8)
        return torch.from_numpy(host).to(dev)[:len(raw)]

    s = torch.cuda.current_stream(dev)

    def timed(fn):
        ts = []
        for i in range(12):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            fn()
            b.record(s)
            torch.cuda.synchronize(dev)
            if i >= 3:
                ts.append(a.elapsed_time(b) * 1e3)
        return {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}

    rows = []
    for K, chunk in cells:
        chunks = syslen_chunks(lines, K, chunk)
        raw = b"".join(chunks)
        starts = np.zeros(K + 1, np.int64)
        starts[1:] = np.cumsum([len(c) for c in chunks])
        d_bytes, d_starts, d_each = to_dev(raw), torch.from_numpy(starts).to(dev), [to_dev(c) for c in chunks]
        cap = len(raw) // 32 + K + 1024
        n_multi = dec.frame_syslen_multi_device(d_bytes, d_starts, cap_frames=cap)[4]
        n_each = sum(dec.frame_syslen_device(d, False, cap_frames=len(c) // 32 + 64)[4] for d, c in zip(d_each, chunks))
        assert n_multi == n_each, (n_multi, n_each)
        multi = timed(lambda: dec.frame_syslen_multi_device(d_bytes, d_starts, cap_frames=cap))
        each = timed(lambda: [dec.frame_syslen_device(d, False, cap_frames=len(c) // 32 + 64) for d, c in zip(d_each, chunks)])
        rows.append({"K": K, "chunk": chunk, "bytes": len(raw), "frames": n_multi, "multi_us": multi, "k_calls_us": each})
        print(f"syslen K={K:5d} chunk={chunk:8d} total={len(raw) / 2**20:7.2f} MiB frames={n_multi}  one launch {multi['median']:.0f} us "
              f"({multi['min']:.0f}..{multi['max']:.0f})  K calls {each['median']:.0f} us ({each['min']:.0f}..{each['max']:.0f})", flush=True)
    raw = syslen_chunks(lines, 1, one_bytes)[0]
    d_bytes, d_starts = to_dev(raw), torch.tensor([0, len(raw)], dtype=torch.int64, device=dev)
    cap = len(raw) // 32 + 1024
    multi = timed(lambda: dec.frame_syslen_multi_device(d_bytes, d_starts, cap_frames=cap))
    single = timed(lambda: dec.frame_syslen_device(d_bytes, False, cap_frames=cap))
    print(f"syslen one stream {len(raw) / 2**20:.2f} MiB  n_segs == 1 {multi['median']:.0f} us ({multi['min']:.0f}..{multi['max']:.0f})  "
          f"single-stream call {single['median']:.0f} us ({single['min']:.0f}..{single['max']:.0f})", flush=True)
    print(json.dumps({"probe": "multi_stream_syslen", "cells": rows, "one_stream": {"bytes": len(raw), "multi_us": multi, "single_us": single}}))


def capnp_chunks(rng, K, chunk):
    """K chunks of about `chunk` bytes: whole messages, then the first words of the next one"""
    import struct

    fills = [b"\0", struct.pack("<2I", 0, 3), struct.pack("<4I", 1, 2, 0, 0), b"some text, ", struct.pack("<2I", 12, 1)]
    out = []
    for _ in range(K):
        buf = bytearray()
        while True:
            words = int(rng.integers(6, 71))
            fill = fills[int(rng.integers(0, len(fills)))]
            m = struct.pack("<2I", 0, words) + (fill * (8 * words // len(fill) + 1))[:8 * words]
            if len(buf) + len(m) > chunk:
                buf += m[:max(8, min(len(m) // 2, chunk - len(buf))) & ~7]
                break
            buf += m
        out.append(bytes(buf))
    return out


def capnp_mode(dev, cells, one_bytes):
    from flowgger_amd import CapnpDecoder

    dec = CapnpDecoder()
    rng = np.random.default_rng(1)

    def to_dev(raw):
        host = np.zeros(((len(raw) + 15) & ~15) + 16, np.uint8)
        host[:len(raw)] = np.frombuffer(raw, np.uint8)
        return torch.from_numpy(host).to(dev)[:len(raw)]

    s = torch.cuda.current_stream(dev)

    def timed(fn):
        ts = []
        for i in range(12):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            fn()
            b.record(s)
            torch.cuda.synchronize(dev)
            if i >= 3:
                ts.append(a.elapsed_time(b) * 1e3)
        return {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}

    rows = []
    for K, chunk in cells:
        chunks = capnp_chunks(rng, K, chunk)
        raw = b"".join(chunks)
        starts = np.zeros(K + 1, np.int64)
        starts[1:] = np.cumsum([len(c) for c in chunks])
        d_bytes, d_starts, d_each = to_dev(raw), torch.from_numpy(starts).to(dev), [to_dev(c) for c in chunks]
        cap = len(raw) // 32 + K + 1024
        n_multi = dec.frame_capnp_multi_device(d_bytes, d_starts, cap_slots=cap)[2] - K  # (every chunk ends in a CARRY slot)
        n_each = sum(dec.frame_capnp_device(d, False, len(c) // 32 + 64)[1] for d, c in zip(d_each, chunks))
        assert n_multi == n_each, (n_multi, n_each)
        multi = timed(lambda: dec.frame_capnp_multi_device(d_bytes, d_starts, cap_slots=cap))
        each = timed(lambda: [dec.frame_capnp_device(d, False, len(c) // 32 + 64) for d, c in zip(d_each, chunks)])
        rows.append({"K": K, "chunk": chunk, "bytes": len(raw), "messages": n_multi, "multi_us": multi, "k_calls_us": each})
        print(f"capnp K={K:5d} chunk={chunk:8d} total={len(raw) / 2**20:7.2f} MiB messages={n_multi}  one launch {multi['median']:.0f} us "
              f"({multi['min']:.0f}..{multi['max']:.0f})  K calls {each['median']:.0f} us ({each['min']:.0f}..{each['max']:.0f})", flush=True)
    raw = capnp_chunks(rng, 1, one_bytes)[0]
    d_bytes, d_starts = to_dev(raw), torch.tensor([0, len(raw)], dtype=torch.int64, device=dev)
    cap = len(raw) // 32 + 1024
    multi = timed(lambda: dec.frame_capnp_multi_device(d_bytes, d_starts, cap_slots=cap))
    single = timed(lambda: dec.frame_capnp_device(d_bytes, False, cap))
    print(f"capnp one stream {len(raw) / 2**20:.2f} MiB  n_segs == 1 {multi['median']:.0f} us ({multi['min']:.0f}..{multi['max']:.0f})  "
          f"single-stream call {single['median']:.0f} us ({single['min']:.0f}..{single['max']:.0f})", flush=True)
    print(json.dumps({"probe": "multi_stream_capnp", "cells": rows, "one_stream": {"bytes": len(raw), "multi_us": multi, "single_us": single}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cells", default=",".join(f"{k}:{c}" for k in (16, 256, 4096) for c in (4 << 10, 64 << 10, 1 << 20)))
    ap.add_argument("--lines", type=int, default=200_000)
    ap.add_argument("--transcode", action="store_true")
    ap.add_argument("--transcode-cells", default=",".join(f"{k}:{c}" for k in (16, 256, 4096) for c in (4 << 10, 64 << 10)))
    ap.add_argument("--syslen", action="store_true")
    ap.add_argument("--syslen-cells", default="64:131072,4096:2048")
    ap.add_argument("--syslen-one", type=int, default=8 << 20)
    ap.add_argument("--capnp", action="store_true")
    ap.add_argument("--capnp-cells", default="64:131072,4096:2048")
    ap.add_argument("--capnp-one", type=int, default=8 << 20)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    if args.capnp:
        capnp_mode(dev, [tuple(int(x) for x in c.split(":")) for c in args.capnp_cells.split(",")], args.capnp_one)
        return
    dec = RFC5424Decoder()
    lines = synth.rfc5424_lines(args.lines, cfg=2)
    if args.syslen:
        lines = [ln if isinstance(ln, bytes) else ln.encode() for ln in lines]
        syslen_mode(dec, lines, dev, [tuple(int(x) for x in c.split(":")) for c in args.syslen_cells.split(",")], args.syslen_one)
        return
    if args.transcode:
        transcode_mode(dec, lines, [tuple(int(x) for x in c.split(":")) for c in args.transcode_cells.split(",")], args.window, args.rounds)
        return
    results = []
    for cell in args.cells.split(","):
        K0, chunk = (int(x) for x in cell.split(":"))
        K = max(1, min(K0, CAP_TOTAL // chunk))
        chunks, counts = build_cell(lines, K, chunk)
        a = SideA(dec, chunks)
        a8 = SideA8(dec, a)
        b = SideB(dec, chunks)
        # the same Records on both sides
        tab, offsets, kind, first = b.tables()
        assert int((kind == L.FG_SLOT_CARRY).sum()) == K
        total = sum(len(c) for c in chunks)
        check = range(K) if total <= (64 << 20) else sorted(set(np.linspace(0, K - 1, 64).astype(int).tolist()))
        for k in check:
            f0, f1 = int(first[k]), int(first[k + 1]) - 1  # (the last slot is the CARRY)
            assert f1 - f0 == counts[k], (k, f1 - f0, counts[k])
            blob, _ = tab.serialize(dec.fmt, b.buf, offsets, f0, f1)
            assert blob.tobytes() == a.rows(k), f"connection {k}: the Records differ"
        assert a.run() == a8.run() == b.run() == sum(counts)
        sides = {"A": a.run, "A8": a8.run, "B": b.run}
        for fn in sides.values():  # warm-up: every shape the windows use
            fn(), fn()
        rates = {s: [] for s in sides}
        per_call = {}
        for _ in range(args.rounds):
            for s, fn in sides.items():
                r, dt = window(fn, args.window)
                rates[s].append(r)
                per_call[s] = dt
        multi, single = frame_only(dec, chunks, dev)
        row = {"K": K, "K_asked": K0, "chunk": chunk, "bytes": total, "lines": sum(counts), "checked_connections": len(check)}
        for s in sides:
            row[s] = {"lines_per_s": statistics.median(rates[s]), "min": min(rates[s]), "max": max(rates[s]), "ms_per_batch": per_call[s] * 1e3}
        row["frame_multi_us"] = {"median": multi[0], "min": multi[1], "max": multi[2]}
        row["frame_single_us"] = {"median": single[0], "min": single[1], "max": single[2]}
        results.append(row)
        print(f"K={K:5d} chunk={chunk:8d} total={total / 2**20:7.1f} MiB  " +
              "  ".join(f"{s} {row[s]['lines_per_s'] / 1e6:7.2f} M lines/s ({row[s]['min'] / 1e6:.2f}..{row[s]['max'] / 1e6:.2f}; {row[s]['ms_per_batch']:.2f} ms)" for s in sides) +
              f"  framing: multi {multi[0]:.0f} us ({multi[1]:.0f}..{multi[2]:.0f}), one stream {single[0]:.0f} us ({single[1]:.0f}..{single[2]:.0f})", flush=True)
        a8.pool.shutdown()
        for d in a8.clones:
            d.close()
        L.lib().fg_free_pinned(a.p)
        L.lib().fg_free_pinned(b.p)
    print(json.dumps({"probe": "multi_stream", "window_s": args.window, "rounds": args.rounds, "cells": results}))


if __name__ == "__main__":
    main()
