#!/usr/bin/env python3
"""Cap'n Proto encoder against the GELF encoder on the same resident tables: the cfg1 RFC5424 corpus is
decoded ONCE (4 M lines: a synth tile replicated on the device), then count + scan + write of each encoder is timed in the same
process, alternating, with device events.  Prints one JSON line: median / min / max ms per call and output bytes per line.
Run the same command under `rocprofv3 --kernel-trace --stats -- python tools/probe/capnp_encode.py` for the per-kernel times."""
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def main():
    import torch

    from flowgger_amd import CapnpEncoder, GelfEncoder, RFC5424Decoder, synth
    from gpu_util import device_path

    n_total = int(sys.argv[1]) if len(sys.argv) > 1 else 4_000_000
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    tile = synth.rfc5424_lines(250_000, cfg=1)
    reps = max(1, n_total // len(tile))
    dec = RFC5424Decoder()
    data, offsets = synth.pack(tile)
    tables, d_bytes, d_offsets = device_path(dec, data, offsets, reps=reps)
    n = len(tile) * reps
    encs = {"capnp": CapnpEncoder(), "gelf": GelfEncoder()}
    outs, times = {}, {k: [] for k in encs}
    for k, e in encs.items():  # sizing + warm-up
        d_out, _ = e.encode_device(dec, d_bytes, d_offsets, n, tables)
        outs[k] = torch.empty(d_out.numel() + 4096, dtype=torch.uint8, device=d_bytes.device)
    torch.cuda.synchronize()
    bytes_out = {}
    for it in range(iters):
        for k, e in (encs.items() if it % 2 == 0 else reversed(list(encs.items()))):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            d_out, _ = e.encode_device(dec, d_bytes, d_offsets, n, tables, out=outs[k])
            b.record()
            torch.cuda.synchronize()
            times[k].append(a.elapsed_time(b))
            bytes_out[k] = d_out.numel()
    res = {"lines": n, "iters": iters}
    for k in encs:
        t = times[k]
        res[k] = {"median_ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3),
                  "bytes_per_line": round(bytes_out[k] / n, 1)}
    print(json.dumps(res))


main()
