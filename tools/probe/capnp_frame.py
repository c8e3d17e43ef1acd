#!/usr/bin/env python3
"""Cap'n Proto stream framing, measured in ONE process on one box.  The stream is what the capnp encoder writes for the cfg2 corpus
(256-byte RFC5424 lines; encoded on the GPU, repeated to --mib):
  (a) fg_frame_capnp_device on the resident stream, ms per GiB of stream
  (b) the host walk on the same bytes, one core: host_walk of csrc/fg_capnp_next.hpp, which is CapnpFramer::frame's loop, compiled
      here with g++ -O2, best of 5, ms per GiB
  (c) fg_frame_decode_batch(FG_FRAME_CAPNP) on the pinned chunk, ms per call
  (d) the route without it: (b) for this stream + fg_decode_batch(FG_CAPNP, FG_FRAME_NONE) on pinned buffers, ms
Usage: capnp_frame.py [--mib N]   -- the driver runs `--step measure` as a child process under its own time limit.  Prints one JSON
line."""
from __future__ import annotations

import ctypes as C
import json
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

WALK_SRC = r'''
#include <chrono>
#include <cstdio>
#include <vector>
#include "fg_capnp_next.hpp"
int main(int argc, char** argv) {
    FILE* f = fopen(argv[1], "rb"); fseek(f, 0, SEEK_END); size_t n = ftell(f); fseek(f, 0, SEEK_SET);
    std::vector<uint8_t> in(n); std::vector<uint64_t> offs; offs.reserve(n / 64);
    if (fread(in.data(), 1, n, f) != n) return 1;
    double best = 1e9;
    for (int rep = 0; rep < 5; ++rep) {
        offs.clear(); uint64_t consumed = 0;
        auto t0 = std::chrono::steady_clock::now();
        fg::capnpf::host_walk(in.data(), n, &consumed, [&](uint64_t p) { offs.push_back(p); });
        double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (consumed != n) return 2;
        if (ms < best) best = ms;
    }
    printf("%.4f\n", best);
}
'''


def stats(xs):
    xs = sorted(xs)
    return [round(xs[0], 4), round(xs[len(xs) // 2], 4), round(xs[-1], 4)]


def measure(mib: int) -> None:
    import numpy as np
    import torch

    from flowgger_amd import CapnpDecoder, CapnpEncoder, RFC5424Decoder, synth
    from flowgger_amd import _lib as L
    from flowgger_amd.tables import DeviceTables

    dev = torch.device("cuda", 0)
    lines = synth.rfc5424_lines(20000, cfg=2)
    data, offsets = synth.pack(lines)
    src = RFC5424Decoder()
    d_bytes = torch.cat([torch.from_numpy(np.ascontiguousarray(data[:int(offsets[-1])])).to(dev), torch.zeros(32, dtype=torch.uint8, device=dev)])
    d_offsets = torch.from_numpy(offsets.astype(np.int64)).to(dev)
    tables = DeviceTables(len(lines), int(offsets[-1]) // 8 + 1024, dev)
    src.decode_device(d_bytes, d_offsets, tables)
    d_out, d_off, _ = CapnpEncoder(None).encode_device(src, d_bytes, d_offsets, len(lines), tables, now_ts=1.5, want_status=True)
    torch.cuda.synchronize(dev)
    tile = d_out[:int(d_off[-1].item())].cpu().numpy()
    reps = max((mib << 20) // tile.size, 1)
    stream = np.tile(tile, reps)
    gib = stream.size / float(1 << 30)
    res = {"bytes": int(stream.size), "messages": len(lines) * reps}

    dec = CapnpDecoder()
    d_stream = torch.cat([torch.from_numpy(stream).to(dev), torch.zeros(32, dtype=torch.uint8, device=dev)])[:stream.size]
    cap = stream.size // 64 + 16
    ts = []
    for k in range(8):
        t0 = time.perf_counter()
        d_offs, n, consumed, stop = dec.frame_capnp_device(d_stream, True, cap)
        torch.cuda.synchronize(dev)
        if k:
            ts.append((time.perf_counter() - t0) * 1e3)
    assert (n, consumed, stop) == (res["messages"], stream.size, L.FG_CAPNP_CLEAN)
    res["a_device_ms_per_gib"] = [round(t / gib, 3) for t in stats(ts)]
    offs = d_offs.cpu().numpy().astype(np.uint64)

    with tempfile.TemporaryDirectory() as td:
        raw, exe, cpp = Path(td) / "stream.bin", Path(td) / "walk", Path(td) / "walk.cpp"
        stream.tofile(raw)
        cpp.write_text(WALK_SRC)
        subprocess.run(["g++", "-O2", "-std=c++17", f"-I{ROOT / 'flowgger_amd' / 'csrc'}", "-o", str(exe), str(cpp)], check=True)
        walk_ms = float(subprocess.run([str(exe), str(raw)], check=True, capture_output=True, text=True, timeout=300).stdout)
    res["b_host_walk_ms_per_gib"] = round(walk_ms / gib, 3)

    pin, pin_off = C.c_void_p(), C.c_void_p()
    L.check(L.lib().fg_alloc_pinned(stream.size + 32, C.byref(pin)), "fg_alloc_pinned")
    L.check(L.lib().fg_alloc_pinned(offs.size * 8, C.byref(pin_off)), "fg_alloc_pinned")
    C.memset(pin, 0, stream.size + 32)
    C.memmove(pin, stream.ctypes.data, stream.size)
    C.memmove(pin_off, offs.ctypes.data, offs.size * 8)
    st, off = L.fg_tables(), C.c_void_p()
    nf, used = C.c_uint64(), C.c_uint64()
    tc, td_ = [], []
    for k in range(8):
        t0 = time.perf_counter()
        L.check(L.lib().fg_frame_decode_batch(dec._ctx, L.FG_CAPNP, L.FG_FRAME_CAPNP, pin, stream.size, 1, C.byref(st), C.byref(off), C.byref(nf),
                                              C.byref(used)), "fg_frame_decode_batch")
        if k:
            tc.append((time.perf_counter() - t0) * 1e3)
    assert nf.value == res["messages"] and L.lib().fg_last_host_path(dec._ctx) == L.FG_PATH_FRAME_CAPNP_DEVICE
    for k in range(8):
        t0 = time.perf_counter()
        L.check(L.lib().fg_decode_batch(dec._ctx, L.FG_CAPNP, pin, stream.size, pin_off, offs.size - 1, C.byref(st)), "fg_decode_batch")
        if k:
            td_.append((time.perf_counter() - t0) * 1e3)
    res["c_frame_decode_batch_ms"] = stats(tc)
    res["d_decode_batch_ms"] = stats(td_)
    res["d_host_walk_plus_decode_ms"] = round(walk_ms + stats(td_)[1], 3)
    L.lib().fg_free_pinned(pin)
    L.lib().fg_free_pinned(pin_off)
    print(json.dumps(res))


def main() -> int:
    args = sys.argv[1:]
    mib = int(args[args.index("--mib") + 1]) if "--mib" in args else 256
    if "--step" in args:
        measure(mib)
        return 0
    return subprocess.run(["timeout", "-k", "10", "420", sys.executable, __file__, "--step", "measure", "--mib", str(mib)]).returncode


if __name__ == "__main__":
    sys.exit(main())
