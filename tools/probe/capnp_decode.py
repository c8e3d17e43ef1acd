#!/usr/bin/env python3
"""Cap'n Proto decode (k_capnp) against the GELF decode of the SAME Records: the cfg1 RFC5424 corpus is decoded
once, encoded on the device as capnp messages and as GELF (a 250 000-line tile each, replicated in HBM to 4 M Records), then the two
decode launches and the float4 copy of fg_calibrate_device over the capnp bytes are timed in one process, alternating, with device
events: 20 repetitions after a warm-up, median.  Prints one JSON line; GB/s = (message bytes read + 68 B per row + 18 B per entry
written) / kernel time.  Under `rocprofv3 --kernel-trace --stats -- python tools/probe/capnp_decode.py` the per-kernel times
(k_capnp; k_gelf + k_gelf_general) come out beside it."""
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def main():
    import torch

    from flowgger_amd import CapnpDecoder, CapnpEncoder, GelfDecoder, GelfEncoder, RFC5424Decoder, synth
    from flowgger_amd import _lib as L
    from flowgger_amd.tables import DeviceTables
    from gpu_util import device_path

    n_total = int(sys.argv[1]) if len(sys.argv) > 1 else 4_000_000
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    tile = synth.rfc5424_lines(250_000, cfg=1)
    reps = max(1, n_total // len(tile))
    src = RFC5424Decoder()
    data, offsets = synth.pack(tile)
    tables, d_bytes, d_offsets = device_path(src, data, offsets)
    dev = d_bytes.device
    n = len(tile) * reps
    legs = {}
    for name, enc, dec in (("capnp", CapnpEncoder(), CapnpDecoder()), ("gelf", GelfEncoder(), GelfDecoder())):
        d_out, d_off = enc.encode_device(src, d_bytes, d_offsets, len(tile), tables)
        torch.cuda.synchronize()
        nb = int(d_off[-1].item())
        assert name != "capnp" or nb % 8 == 0
        big = torch.cat([d_out[:nb].repeat(reps), torch.zeros(32, dtype=torch.uint8, device=dev)])
        o = d_off[:-1].to(torch.int64)
        base = torch.arange(reps, device=dev, dtype=torch.int64).repeat_interleave(len(tile)) * nb
        offs = torch.cat([o.repeat(reps) + base, torch.tensor([nb * reps], device=dev, dtype=torch.int64)])
        t = DeviceTables(n, nb * reps // 8 + 1024, dev)
        legs[name] = (dec, big, offs, t, nb * reps)
    times = {k: [] for k in list(legs) + ["copy"]}
    dec_c, big_c, _, _, nbytes_c = legs["capnp"]
    dst = torch.empty(nbytes_c + 32, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev)

    def run(k):
        if k == "copy":
            L.check(L.lib().fg_calibrate_device(dec_c._ctx, 0, big_c.data_ptr(), dst.data_ptr(), nbytes_c, C.c_void_p(stream.cuda_stream)), "fg_calibrate_device")
        else:
            dec, big, offs, t, _ = legs[k]
            dec.decode_device(big, offs, t)

    for k in times:  # warm-up
        run(k)
    torch.cuda.synchronize()
    order = list(times)
    for it in range(iters):
        for k in (order if it % 2 == 0 else reversed(order)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run(k)
            b.record()
            torch.cuda.synchronize()
            times[k].append(a.elapsed_time(b))
    res = {"records": n, "iters": iters}
    for k in legs:
        dec, big, offs, t, nbytes = legs[k]
        ok = int((t.column("meta").view(torch.int32) & 0xFF).eq(0).sum().item())
        ents = int(t.column("ent_count").view(torch.int32).sum().item())
        ms = statistics.median(times[k])
        res[k] = {"median_ms": round(ms, 3), "min_ms": round(min(times[k]), 3), "max_ms": round(max(times[k]), 3), "ok_rows": ok,
                  "bytes_per_record": round(nbytes / n, 1), "entries": ents,
                  "GBps": round((nbytes + 68 * n + 18 * ents) / ms / 1e6, 1), "ns_per_record": round(ms * 1e6 / n, 3)}
    ms = statistics.median(times["copy"])
    res["copy"] = {"median_ms": round(ms, 3), "min_ms": round(min(times["copy"]), 3), "max_ms": round(max(times["copy"]), 3),
                   "GBps": round(2 * nbytes_c / ms / 1e6, 1)}
    print(json.dumps(res))


main()
