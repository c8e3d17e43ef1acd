#!/usr/bin/env python3
"""The UDP input's inflate on the device, measured (nothing here is gated): GELF lines, each compressed on its own with zlib at
level 6, resident in HBM.  In ONE process on one box:
  (a) every stage of fg_udp_unpack_device under HIP events -- count, scan, write, finish (bare-record copy + UTF-8) -- 20 runs after
      3 warm-ups, median and spread; datagrams/s, compressed GB/s in and inflated GB/s out per stage
  (b) the same datagrams through Python's zlib on one core of the same box
  (c) fg_udp_decode_batch on the datagrams against fg_decode_batch on the already-inflated lines (pinned host buffers, wall clock)
With --once, (a) alternates run by run with the one-walk unpacker of fg_udp_unpack_once_device -- stage (capacities, their scan, the
walk, the scan of the sizes), the write walk of the spilled rows, pack -- and reports both sides' stages, the per-run totals (median,
min .. max: the two ranges are what the decision between the forms rests on) and the spilled share; and (c) also runs
fg_udp_transcode_batch against fg_udp_decode_batch on the same pinned datagrams, with the bytes each sends over the link each way.
Usage: udp_inflate.py [--n 1000000] [--unique 20000] [--once]   -- prints one JSON line."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
import time
import zlib
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


def dec_spilled(lib, dec):
    lib.fg_udp_last_spilled.restype = C.c_uint64
    return int(lib.fg_udp_last_spilled(dec._ctx))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--unique", type=int, default=20_000)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    import torch

    from flowgger_amd import GelfDecoder, synth
    from flowgger_amd import _lib as L

    lines = [bytes(l).rstrip(b"\n") for l in synth.gelf_lines(a.unique, invalid_frac=0.0)]
    grams = [zlib.compress(l, 6) for l in lines]
    reps = max(1, a.n // len(grams))
    n = reps * len(grams)
    sizes = np.tile(np.array([len(g) for g in grams], np.uint64), reps)
    offs = np.zeros(n + 1, np.uint64)
    offs[1:] = np.cumsum(sizes)
    blob = np.tile(np.frombuffer(b"".join(grams), np.uint8), reps)
    lsizes = np.tile(np.array([len(l) for l in lines], np.uint64), reps)
    loffs = np.zeros(n + 1, np.uint64)
    loffs[1:] = np.cumsum(lsizes)
    lblob = np.tile(np.frombuffer(b"".join(lines), np.uint8), reps)
    in_bytes, out_bytes = int(offs[-1]), int(loffs[-1])

    dec = GelfDecoder()
    lib = L.lib()
    dev = torch.device("cuda", dec.device)
    pad = lambda x: np.concatenate([x, np.zeros(32 - x.size % 16, np.uint8)])
    d_bytes = torch.from_numpy(pad(blob)).to(dev)
    d_offs = torch.from_numpy(offs.astype(np.int64)).to(dev)
    d_sizes = torch.zeros(n + 4, dtype=torch.int32, device=dev)
    d_sums = torch.zeros((n + 63) // 64 + 1, dtype=torch.int64, device=dev)
    d_st = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_drop = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_ooff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_out = torch.zeros((out_bytes + 15) // 16 * 16 + 16, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev)
    sp = C.c_void_p(stream.cuda_stream)
    vp, u64 = C.c_void_p, C.c_uint64
    lib.fg_launch_udp_count.argtypes = [vp, vp, u64, C.c_uint32, vp, vp, vp, vp, vp]
    lib.fg_launch_encode_scan.argtypes = [vp, vp, u64, vp, u64, vp]
    for f in (lib.fg_launch_udp_write, lib.fg_launch_udp_finish):
        f.argtypes = [vp, vp, u64, vp, vp, u64, vp, vp, vp]
    stages = {
        "count": lambda: lib.fg_launch_udp_count(d_bytes.data_ptr(), d_offs.data_ptr(), n, L.FG_UDP_DEFAULT_MAX_INFLATED, d_sizes.data_ptr(),
                                                 d_sums.data_ptr(), d_st.data_ptr(), d_drop.data_ptr(), sp),
        "scan": lambda: lib.fg_launch_encode_scan(d_sizes.data_ptr(), d_sums.data_ptr(), n, d_ooff.data_ptr(), 0, sp),
        "write": lambda: lib.fg_launch_udp_write(d_bytes.data_ptr(), d_offs.data_ptr(), n, d_ooff.data_ptr(), d_out.data_ptr(), out_bytes,
                                                 d_st.data_ptr(), d_drop.data_ptr(), sp),
        "utf8": lambda: lib.fg_launch_udp_finish(d_bytes.data_ptr(), d_offs.data_ptr(), n, d_ooff.data_ptr(), d_out.data_ptr(), out_bytes,
                                                 d_st.data_ptr(), d_drop.data_ptr(), sp),
    }
    once = {}
    if a.once:
        lib.fg_udp_stage_bytes.argtypes, lib.fg_udp_stage_bytes.restype = [u64, u64], u64
        lib.fg_launch_udp_stage.argtypes = [vp, vp, u64, C.c_uint32, vp, vp, vp, vp, u64, vp, vp, vp, vp, vp, vp, vp, vp]
        lib.fg_launch_udp_write_spilled.argtypes = [vp, vp, u64, vp, vp, u64, vp, vp, vp, vp]
        lib.fg_launch_udp_pack.argtypes = [vp, vp, u64, vp, vp, u64, vp, vp, vp, vp, u64, vp, vp]
        stage_cap = int(lib.fg_udp_stage_bytes(in_bytes, n))
        d_stage = torch.zeros(stage_cap, dtype=torch.uint8, device=dev)
        d_wsz = torch.zeros(n + 4, dtype=torch.int32, device=dev)
        d_wsums = torch.zeros((n + 63) // 64 + 1, dtype=torch.int64, device=dev)
        d_woff = torch.zeros(n + 2, dtype=torch.int64, device=dev)
        d_sizes1 = torch.zeros(n + 4, dtype=torch.int32, device=dev)
        d_sums1 = torch.zeros((n + 63) // 64 + 1, dtype=torch.int64, device=dev)
        d_st1, d_drop1, d_spl = (torch.zeros(n, dtype=torch.uint8, device=dev) for _ in range(3))
        d_nspl = torch.zeros(4, dtype=torch.int32, device=dev)
        d_ooff1 = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        d_out1 = torch.zeros((out_bytes + 15) // 16 * 16 + 16, dtype=torch.uint8, device=dev)
        once = {
            "once_stage": lambda: lib.fg_launch_udp_stage(d_bytes.data_ptr(), d_offs.data_ptr(), n, L.FG_UDP_DEFAULT_MAX_INFLATED, d_wsz.data_ptr(),
                                                          d_wsums.data_ptr(), d_woff.data_ptr(), d_stage.data_ptr(), stage_cap, d_sizes1.data_ptr(),
                                                          d_sums1.data_ptr(), d_ooff1.data_ptr(), d_st1.data_ptr(), d_drop1.data_ptr(), d_spl.data_ptr(),
                                                          d_nspl.data_ptr(), sp),
            # (as fg_udp_once_pack: launched only when a row spilled; the count is read after the stage, outside the timed spans)
            "once_write_spilled": lambda: lib.fg_launch_udp_write_spilled(d_bytes.data_ptr(), d_offs.data_ptr(), n, d_ooff1.data_ptr(), d_out1.data_ptr(),
                                                                          out_bytes, d_st1.data_ptr(), d_drop1.data_ptr(), d_spl.data_ptr(), sp)
            if int(d_nspl[0].item()) else 0,
            "once_pack": lambda: lib.fg_launch_udp_pack(d_bytes.data_ptr(), d_offs.data_ptr(), n, d_ooff1.data_ptr(), d_out1.data_ptr(), out_bytes,
                                                        d_st1.data_ptr(), d_drop1.data_ptr(), d_stage.data_ptr(), d_woff.data_ptr(), stage_cap, d_spl.data_ptr(), sp),
        }
    ms = {k: [] for k in list(stages) + list(once)}
    for run in range(a.warmup + a.runs):
        for k, fn in list(stages.items()) + list(once.items()):  # (the two sides alternate run by run)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            assert fn() == 0, k
            e1.record(stream)
            e1.synchronize()
            if run >= a.warmup:
                ms[k].append(e0.elapsed_time(e1))
    assert int(d_ooff[-1].item()) == out_bytes and int(d_drop.sum().item()) == 0
    assert bool((d_out[:out_bytes].cpu() == torch.from_numpy(lblob)).all()), "the inflated bytes differ from the lines"
    res = {"n": n, "unique": len(grams), "compressed_bytes": in_bytes, "inflated_bytes": out_bytes, "stages": {}}
    for k, v in ms.items():
        s = spread(v)
        t = s["median_ms"] / 1e3
        s.update({"datagrams_per_s": round(n / t), "compressed_GBps_in": round(in_bytes / t / 1e9, 3), "inflated_GBps_out": round(out_bytes / t / 1e9, 3)})
        res["stages"][k] = s
    tot = sum(statistics.median(ms[k]) for k in stages) / 1e3
    res["unpack_total"] = {"ms": round(tot * 1e3, 3), "datagrams_per_s": round(n / tot), "inflated_GBps_out": round(out_bytes / tot / 1e9, 3)}
    if a.once:
        assert int(d_ooff1[-1].item()) == out_bytes and int(d_drop1.sum().item()) == 0
        assert bool((d_out1[:out_bytes].cpu() == torch.from_numpy(lblob)).all()), "the one-walk form's bytes differ from the lines"
        per_run = lambda keys: [sum(ms[k][r] for k in keys) for r in range(a.runs)]
        res["two_walk_total"] = spread(per_run(list(stages)))
        res["one_walk_total"] = spread(per_run(list(once)))
        res["spilled"] = {"datagrams": int(d_nspl[0].item()), "share": round(int(d_nspl[0].item()) / n, 6), "stage_bytes": stage_cap}
    # (b) Python zlib, one core
    t0 = time.perf_counter()
    for g in grams:
        zlib.decompress(g)
    tz = (time.perf_counter() - t0) / len(grams)
    res["zlib_one_core"] = {"datagrams_per_s": round(1 / tz), "inflated_GBps_out": round(out_bytes / n / tz / 1e9, 4)}
    # (c) host-buffer calls, pinned
    keep = []
    pb, p1 = pinned(pad(blob)); po, p2 = pinned(offs); plb, p3 = pinned(pad(lblob)); plo, p4 = pinned(loffs)
    keep += [p1, p2, p3, p4]
    wall = {"fg_udp_decode_batch": [], "fg_decode_batch": []}
    for run in range(2 + 5):
        t0 = time.perf_counter()
        dec.udp_decode_packed(pb[:in_bytes], po)
        t1 = time.perf_counter()
        dec.decode_packed(plb[:out_bytes], plo)
        t2 = time.perf_counter()
        if run >= 2:
            wall["fg_udp_decode_batch"].append((t1 - t0) * 1e3)
            wall["fg_decode_batch"].append((t2 - t1) * 1e3)
    res["host_buffer_calls"] = {k: spread(v) for k, v in wall.items()}
    if a.once:
        from flowgger_amd import GelfEncoder, Pipeline

        pipe = Pipeline(dec, GelfEncoder(None, merger="line"))
        wall2 = {"fg_udp_transcode_batch": [], "fg_udp_decode_batch": []}
        for run in range(2 + 5):
            t0 = time.perf_counter()
            t = pipe.run_datagrams((pb[:in_bytes], po))
            t1 = time.perf_counter()
            tab, ulines, uoffs, ust = dec.udp_decode_packed(pb[:in_bytes], po)
            t2 = time.perf_counter()
            if run >= 2:
                wall2["fg_udp_transcode_batch"].append((t1 - t0) * 1e3)
                wall2["fg_udp_decode_batch"].append((t2 - t1) * 1e3)
        up = in_bytes + (n + 1) * 8
        res["transcode_vs_decode"] = {k: spread(v) for k, v in wall2.items()}
        res["transcode_vs_decode"]["link_bytes"] = {
            "fg_udp_transcode_batch": {"up": up, "down": int(t.out.size) + (n + 1) * 8 + n * 4 + n + n},
            "fg_udp_decode_batch": {"up": up, "down": int(uoffs[-1]) + (n + 1) * 8 + n + sum(int(v.nbytes) for v in tab.a.values())}}
        res["transcode_vs_decode"]["note"] = "both wrappers also copy what came back into numpy arrays on the host; the tables are counted with their entry columns at capacity; spilled: %d" % dec_spilled(lib, dec)
    res["host_buffer_calls"]["note"] = "udp_decode_packed also copies the inflated lines into a numpy array on the host"
    for p in keep:
        lib.fg_free_pinned(p)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
