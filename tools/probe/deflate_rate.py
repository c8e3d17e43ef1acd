#!/usr/bin/env python3
"""The output compressor on the device, measured (nothing here is gated).  In ONE process on one box:
  (a) fg_deflate_device alone on a resident GELF-encoded stream of about --mib MiB (what the GELF encoder made of RFC5424 lines, tiled),
      cut into members of one message, about 4 KiB and about 64 KiB: wall clock around the call (it synchronises), --runs runs after
      --warmup warm-ups, median and spread; input GB/s, compressed / raw
  (b) fg_transcode_batch on --lines RFC5424 lines -> GELF from pinned host buffers: compression off in its pipelined (sliced) form, off in
      one piece (the path compression takes), gzip with member_bytes 65536; lines/s, and the bytes each form sends down the link
  (c) fg_measure_link's rates in the same process
--huffman fixed | dynamic | both (the default): fg_set_deflate_mode for (a) and for the gzip leg of (b); with both, every figure of the
compressor is taken in either mode in the same process, the fixed mode first (its keys are the ones this tool always had, the dynamic
mode's carry "_dynamic").
Usage: deflate_rate.py [--mib 256] [--lines 4000000] [--unique 100000] [--huffman both]   -- prints one JSON line."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def pinned(arr):
    from flowgger_amd import _lib as L

    p = C.c_void_p()
    L.check(L.lib().fg_alloc_pinned(arr.nbytes + 32, C.byref(p)), "fg_alloc_pinned")
    view = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), (arr.nbytes + 32,))
    view[:arr.nbytes] = arr.view(np.uint8).reshape(-1)
    return view[:arr.nbytes].view(arr.dtype), p


def cuts_by_bytes(off, b):
    """fg_compress_cfg's member_bytes policy over out_offsets"""
    blk = off[:-1] // np.uint64(b)
    starts = np.concatenate([[True], blk[1:] > blk[:-1]])
    return np.concatenate([off[:-1][starts], off[-1:]]).astype(np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--lines", type=int, default=4_000_000)
    ap.add_argument("--unique", type=int, default=100_000)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--huffman", choices=("fixed", "dynamic", "both"), default="both")
    a = ap.parse_args()
    import torch

    from flowgger_amd import Encoder, GelfEncoder, Pipeline, RFC5424Decoder, synth
    from flowgger_amd import _lib as L

    lib = L.lib()
    dec = RFC5424Decoder()
    dev = torch.device("cuda", dec.device)
    enc = GelfEncoder(None, merger="line")
    lines = synth.rfc5424_lines(a.unique, cfg=2)
    data, offsets = synth.pack(lines)
    res = {"block_bytes": int(lib.fg_deflate_block_bytes())}
    modes = ("fixed", "dynamic") if a.huffman == "both" else (a.huffman,)
    key = lambda name, mode: name + ("_dynamic" if mode == "dynamic" and a.huffman == "both" else "")

    # (a) the compressor alone
    t = Pipeline(dec, enc).run_packed(data, offsets)
    unit, unit_off = t.out, t.out_offsets
    reps = max(1, (a.mib << 20) // unit.size)
    stream = np.tile(unit, reps)
    base = (np.arange(reps, dtype=np.uint64) * np.uint64(unit.size)).repeat(len(unit_off) - 1)
    off = np.concatenate([np.tile(unit_off[:-1], reps) + base, [np.uint64(stream.size)]]).astype(np.uint64)
    d_bytes = torch.from_numpy(stream).to(dev)
    d_out = torch.empty(int(lib.fg_deflate_bound(stream.size, len(off) - 1)) + 64, dtype=torch.uint8, device=dev)
    res["deflate_device"] = {"input_bytes": int(stream.size), "messages": len(off) - 1}
    for name, cuts in (("one_message", off), ("4KiB", cuts_by_bytes(off, 4096)), ("64KiB", cuts_by_bytes(off, 65536))):
        d_cuts = torch.from_numpy(cuts.astype(np.int64)).to(dev)
        for mode in modes:
            ms = []
            for run in range(a.warmup + a.runs):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                d_z, d_zoff = Encoder.deflate_device(dec, d_bytes, d_cuts, out=d_out, huffman=mode)
                t1 = time.perf_counter()
                if run >= a.warmup:
                    ms.append((t1 - t0) * 1e3)
            s = spread(ms)
            s.update({"members": len(cuts) - 1, "input_GBps": round(stream.size / (s["median_ms"] / 1e3) / 1e9, 3), "compressed_bytes": int(d_z.numel()),
                      "ratio": round(int(d_z.numel()) / stream.size, 4)})
            res["deflate_device"][key(name, mode)] = s
        del d_cuts
    del d_bytes, d_out, stream, off

    # (b) fg_transcode_batch, pinned host buffers, no copies on the host
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

    def call():
        L.check(lib.fg_transcode_batch(dec._ctx, dec.fmt, L.FG_FRAME_NONE, C.byref(cfg), pb.ctypes.data, nbytes, po.ctypes.data, n, 1, C.byref(out)),
                "fg_transcode_batch")

    def leg(one_piece, gzip, mode="fixed"):
        dec.set_launch_opts(transcode_one_piece=one_piece)
        L.check(lib.fg_set_deflate_mode(dec._ctx, L.FG_DEFLATE_DYNAMIC if mode == "dynamic" else L.FG_DEFLATE_FIXED), "fg_set_deflate_mode")
        cc = L.fg_compress_cfg(L.FG_COMP_GZIP if gzip else L.FG_COMP_NONE, 0, 65536)
        L.check(lib.fg_set_output_compression(dec._ctx, C.byref(cc)), "fg_set_output_compression")
        ms = []
        for run in range(a.warmup + a.runs):
            t0 = time.perf_counter()
            call()
            t1 = time.perf_counter()
            if run >= a.warmup:
                ms.append((t1 - t0) * 1e3)
        s = spread(ms)
        L.check(lib.fg_last_compressed(dec._ctx, C.byref(comp)), "fg_last_compressed")
        fixed = (n + 1) * 8 + n * 4 + n
        down = (int(comp.z_bytes) + 16 * (int(comp.n_members) + 1) if gzip else int(out.out_bytes)) + fixed
        s.update({"lines_per_s": round(n / (s["median_ms"] / 1e3)), "down_bytes": down, "out_bytes": int(out.out_bytes)})
        if gzip:
            s.update({"z_bytes": int(comp.z_bytes), "members": int(comp.n_members), "ratio": round(int(comp.z_bytes) / int(comp.raw_bytes), 4)})
        return s

    res["transcode_batch"] = {"lines": n, "input_bytes": nbytes}
    res["transcode_batch"]["off_sliced"] = leg(False, False)
    res["transcode_batch"]["off_one_piece"] = leg(True, False)
    for mode in modes:
        res["transcode_batch"][key("gzip_64KiB_one_piece", mode)] = leg(True, True, mode)
    res["transcode_batch"]["off_sliced_again"] = leg(False, False)  # (the first leg once more: drift over the run)
    # (c) the link, same process
    g = (C.c_double * 3)()
    L.check(lib.fg_measure_link(dec._ctx, 256 << 20, g), "fg_measure_link")
    res["link_GBps"] = {"h2d": round(g[0], 2), "d2h": round(g[1], 2), "both": round(g[2], 2)}
    for p in (p1, p2):
        lib.fg_free_pinned(p)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
