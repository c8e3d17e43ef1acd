#!/usr/bin/env python3
"""Kafka v0 message sets on the device, measured (nothing here is gated).  In ONE process on one box, the method of deflate_rate.py
(wall clock around a call that synchronises, --runs runs after --warmup warm-ups, median and spread):
  (a) fg_kafka_messageset_device alone on a resident GELF-encoded stream of about --mib MiB (what the GELF encoder made of RFC5424 lines,
      tiled): ms and input GB/s, and beside it fg_calibrate_device(FG_CALIB_COPY) over the same byte count -- the roof of a pass that
      reads and writes every byte once; `of_copy` = the copy's time over the set's
  (b) fg_kafka_wrap_device over the gzip members fg_deflate_device makes of that set, members of one message, about 4 KiB and about 64 KiB
  (c) fg_transcode_batch on --lines RFC5424 lines -> GELF from pinned host buffers, gzip, member_bytes 65536, with wire = raw and with
      wire = kafka: the difference is what the message sets cost
Usage: kafka_rate.py [--mib 256] [--lines 4000000] [--unique 100000]   -- prints one JSON line."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from deflate_rate import cuts_by_bytes, pinned, spread  # noqa: E402


def timed(fn, sync, warmup, runs):
    ms = []
    for run in range(warmup + runs):
        sync()
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        if run >= warmup:
            ms.append((t1 - t0) * 1e3)
    return spread(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--lines", type=int, default=4_000_000)
    ap.add_argument("--unique", type=int, default=100_000)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch

    from flowgger_amd import Encoder, GelfEncoder, Pipeline, RFC5424Decoder, synth
    from flowgger_amd import _lib as L

    lib = L.lib()
    dec = RFC5424Decoder()
    dev = torch.device("cuda", dec.device)
    sync = lambda: torch.cuda.synchronize(dev)
    enc = GelfEncoder(None, merger="line")
    lines = synth.rfc5424_lines(a.unique, cfg=2)
    data, offsets = synth.pack(lines)
    res = {}

    # (a) the set alone, and the copy
    t = Pipeline(dec, enc).run_packed(data, offsets)
    unit, unit_off, unit_skip = t.out, t.out_offsets, (t.enc_status != 0).astype(np.uint8)
    reps = max(1, (a.mib << 20) // unit.size)
    stream = np.tile(unit, reps)
    base = (np.arange(reps, dtype=np.uint64) * np.uint64(unit.size)).repeat(len(unit_off) - 1)
    off = np.concatenate([np.tile(unit_off[:-1], reps) + base, [np.uint64(stream.size)]]).astype(np.uint64)
    n = len(off) - 1
    d_bytes = torch.from_numpy(stream).to(dev)
    d_off = torch.from_numpy(off.astype(np.int64)).to(dev)
    d_skip = torch.from_numpy(np.tile(unit_skip, reps)).to(dev)
    d_set = torch.empty(stream.size + 26 * n + 64, dtype=torch.uint8, device=dev)
    box = {}

    def build():
        box["set"] = Encoder.kafka_messageset_device(dec, d_bytes, d_off, d_skip, out=d_set)

    s = timed(build, sync, a.warmup, a.runs)
    s.update({"input_bytes": int(stream.size), "messages": n, "set_bytes": int(box["set"][0].numel()),
              "input_GBps": round(stream.size / (s["median_ms"] / 1e3) / 1e9, 3)})
    res["messageset_device"] = s
    d_dst = torch.empty(stream.size + 64, dtype=torch.uint8, device=dev)
    nb = stream.size & ~15

    def copy():
        L.check(lib.fg_calibrate_device(dec._ctx, 0, d_bytes.data_ptr(), d_dst.data_ptr(), nb, None), "fg_calibrate_device")
        sync()

    c = timed(copy, sync, a.warmup, a.runs)
    c.update({"bytes": int(nb), "GBps": round(nb / (c["median_ms"] / 1e3) / 1e9, 3)})
    res["calib_copy"] = c
    res["messageset_device"]["of_copy"] = round(c["median_ms"] / s["median_ms"], 3)
    del d_dst

    # (b) the wrap at three member sizes
    d_s, d_soff = box["set"]
    soff = d_soff.cpu().numpy().astype(np.uint64)
    d_z = torch.empty(int(lib.fg_deflate_bound(d_s.numel(), n)) + 64, dtype=torch.uint8, device=dev)
    d_w = torch.empty(int(lib.fg_kafka_bound(stream.size, n, n)) + 64, dtype=torch.uint8, device=dev)
    res["wrap_device"] = {}
    for name, first_cuts in (("one_message", off), ("4KiB", cuts_by_bytes(off, 4096)), ("64KiB", cuts_by_bytes(off, 65536))):
        first = np.searchsorted(off, first_cuts, side="left")  # (the members' first messages; offsets of equal value: the first of them)
        d_cuts = torch.from_numpy(soff[first].astype(np.int64)).to(dev)
        zz, d_zoff = Encoder.deflate_device(dec, d_s, d_cuts, out=d_z)

        def wrap():
            box["w"] = Encoder.kafka_wrap_device(dec, zz, d_zoff, out=d_w)

        w = timed(wrap, sync, a.warmup, a.runs)
        w.update({"members": len(first) - 1, "z_bytes": int(zz.numel()), "wrapped_bytes": int(box["w"][0].numel()),
                  "z_GBps": round(int(zz.numel()) / (w["median_ms"] / 1e3) / 1e9, 3)})
        res["wrap_device"][name] = w
        del d_cuts
    del d_bytes, d_set, d_z, d_w, d_s, stream, off, box

    # (c) fg_transcode_batch, pinned host buffers, gzip by 64 KiB, raw and kafka
    reps = max(1, a.lines // len(lines))
    n = reps * len(lines)
    sizes = np.tile(np.diff(offsets.astype(np.int64)).astype(np.uint64), reps)
    offs = np.zeros(n + 1, np.uint64)
    offs[1:] = np.cumsum(sizes)
    blob = np.tile(data[:int(offsets[-1])], reps)
    nbytes = int(offs[-1])
    pb, p1 = pinned(blob)
    po, p2 = pinned(offs)
    del blob
    cfg, _keep = enc._cfg_struct(0.0)
    out = L.fg_transcoded()
    comp = L.fg_compressed()
    cc = L.fg_compress_cfg(L.FG_COMP_GZIP, 0, 65536)
    L.check(lib.fg_set_output_compression(dec._ctx, C.byref(cc)), "fg_set_output_compression")
    L.check(lib.fg_set_deflate_mode(dec._ctx, L.FG_DEFLATE_FIXED), "fg_set_deflate_mode")

    def call():
        L.check(lib.fg_transcode_batch(dec._ctx, dec.fmt, L.FG_FRAME_NONE, C.byref(cfg), pb.ctypes.data, nbytes, po.ctypes.data, n, 1, C.byref(out)),
                "fg_transcode_batch")

    res["transcode_batch"] = {"lines": n, "input_bytes": nbytes}
    for name, wire in (("gzip_64KiB_raw", L.FG_WIRE_RAW), ("gzip_64KiB_kafka", L.FG_WIRE_KAFKA_V0), ("gzip_64KiB_raw_again", L.FG_WIRE_RAW)):
        L.check(lib.fg_set_output_wire(dec._ctx, wire), "fg_set_output_wire")
        s = timed(call, lambda: None, a.warmup, a.runs)
        L.check(lib.fg_last_compressed(dec._ctx, C.byref(comp)), "fg_last_compressed")
        s.update({"lines_per_s": round(n / (s["median_ms"] / 1e3)), "z_bytes": int(comp.z_bytes), "members": int(comp.n_members),
                  "out_bytes": int(out.out_bytes)})
        res["transcode_batch"][name] = s
    for p in (p1, p2):
        lib.fg_free_pinned(p)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
