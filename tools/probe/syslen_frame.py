#!/usr/bin/env python3
"""Octet-counted framing on the device, measured: for the cfg2 corpus (256-byte RFC5424 lines) and the long-tail corpus wrapped as
syslen, in ONE process on one box:
  (a) fg_frame_syslen_device, resident stream: frame + pack, ms per GiB of stream
  (b) the one-pass `line` framer (fg_frame_device) on the same payloads
  (c) the host hop on the same bytes, one core: the Syslen branch of fg::BatchingSplitter::run (host/fg_decoder.hpp) -- its own
      BufferedSource::get() / read_exact(), the UTF-8 check and the copy into the batch buffer, without the decode of a full batch --
      compiled here with g++ -O2; beside it (c2) the host hop the host-buffer entry points fall back to (host_walk of
      csrc/fg_syslen_parse.hpp + a copy of every message)
  (d) fg_frame_decode_batch(FG_FRAME_SYSLEN) on a pinned chunk against the route without it: (c), then fg_decode_batch on pinned buffers
Usage: syslen_frame.py [--mib N]   -- the driver: runs `--step check` and then `--step measure`, each a child process under its own
time limit, the second only when the first succeeded.  Prints one JSON line per corpus."""
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

HOP_SRC = r'''
#include <chrono>
#include <cstdio>
#include <cstring>
#include <vector>
#include "fg_syslen_parse.hpp"
int main(int argc, char** argv) {
    FILE* f = fopen(argv[1], "rb"); fseek(f, 0, SEEK_END); size_t n = ftell(f); fseek(f, 0, SEEK_SET);
    std::vector<uint8_t> in(n), out(n); std::vector<uint64_t> offs; offs.reserve(n / 32);
    if (fread(in.data(), 1, n, f) != n) return 1;
    double best = 1e9;
    for (int rep = 0; rep < 5; ++rep) {
        offs.assign(1, 0); uint64_t consumed = 0, w = 0;
        auto t0 = std::chrono::steady_clock::now();
        fg::syslen::host_walk(in.data(), n, ~0ull, &consumed, [&](uint64_t pos, uint32_t plen, uint64_t len) {
            memcpy(out.data() + w, in.data() + pos + plen, len); w += len; offs.push_back(w); });
        double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (consumed != n) return 2;
        if (ms < best) best = ms;
    }
    printf("%.4f\n", best);
}
'''

SPLITTER_HOP_SRC = r'''
#include <chrono>
#include <cstdio>
#include <fstream>
#include "fg_decoder.hpp"
int main(int argc, char** argv) {
    double best = 1e9;
    for (int rep = 0; rep < 3; ++rep) {
        std::ifstream f(argv[1], std::ios::binary);
        fg::IstreamSource src(f);
        fg::FlushPolicy pol;
        fg::BufferedSource in(src, pol);
        std::vector<uint8_t> bytes; std::vector<uint64_t> offs{0};
        in.on_block([&] { return bytes.size(); }, [&] {});
        std::string line; uint64_t frames = 0;
        auto t0 = std::chrono::steady_clock::now();
        for (;;) {  // the Syslen branch of fg::BatchingSplitter::run, without the decode of a full batch
            std::string num; int c;
            while ((c = in.get()) >= 0 && c != ' ') num.push_back((char)c);
            if (c < 0) break;
            size_t len = 0, k = (!num.empty() && num[0] == '+') ? 1 : 0; bool ok = k < num.size();
            for (; k < num.size() && ok; ++k) { if (num[k] < '0' || num[k] > '9' || len > (SIZE_MAX - 9) / 10) ok = false; else len = len * 10 + (size_t)(num[k] - '0'); }
            if (!ok) return 2;
            line.clear();
            if (in.read_exact(line, len) != len) return 3;
            if (!fg::detail::valid_utf8((const uint8_t*)line.data(), line.size())) continue;  // (the splitter ends here; the probe's corpora have none)
            bytes.insert(bytes.end(), line.begin(), line.end());
            offs.push_back(bytes.size());
            ++frames;
        }
        double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (ms < best) best = ms;
        if (!frames) return 5;
    }
    printf("%.4f\n", best);
}
'''


def wrap(lines):
    return b"".join(b"%d %s\n" % (len(m) + 1, m if isinstance(m, bytes) else m.encode()) for m in lines)


def corpora(mib):
    from flowgger_amd import synth

    out = {}
    for name, lines in (("cfg2", synth.rfc5424_lines(20000, cfg=2)), ("long_tail", synth.rfc5424_lines(8000, cfg=5, long_tail=True))):
        one = wrap(lines)
        out[name] = one * max(1, (mib << 20) // len(one))
    return out


def best_ms(fn, reps=7):
    import torch

    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[0], ts[len(ts) // 2], ts[-1]


def wall_ms(fn, reps=7):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[0], ts[len(ts) // 2], ts[-1]


def pinned_copy(L, data: bytes):
    p = C.c_void_p()
    L.check(L.lib().fg_alloc_pinned(len(data) + 32, C.byref(p)), "fg_alloc_pinned")
    C.memset(p, 0, len(data) + 32)
    C.memmove(p, data, len(data))
    return p


def step_check():
    import torch
    from flowgger_amd import RFC5424Decoder, synth

    dec = RFC5424Decoder()
    raw = wrap(synth.rfc5424_lines(1000, cfg=2))
    buf = torch.zeros((len(raw) + 31) // 16 * 16, dtype=torch.uint8, device="cuda")
    buf[:len(raw)] = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
    r = dec.frame_syslen_device(buf[:len(raw)])
    assert r[4] == 1000 and r[5] == len(raw) and r[6] == 0, r[4:]
    print("check ok")


def step_measure(mib):
    import numpy as np
    import torch
    from flowgger_amd import RFC5424Decoder
    from flowgger_amd import _lib as L

    with tempfile.TemporaryDirectory() as td:
        exe = Path(td) / "hop"
        (Path(td) / "hop.cpp").write_text(HOP_SRC)
        subprocess.run(["g++", "-O2", "-std=c++17", f"-I{ROOT / 'flowgger_amd' / 'csrc'}", "-o", str(exe), str(Path(td) / "hop.cpp")], check=True)
        exe2 = Path(td) / "splitter_hop"
        (Path(td) / "splitter_hop.cpp").write_text(SPLITTER_HOP_SRC)
        subprocess.run(["g++", "-O2", "-std=c++17", f"-I{ROOT / 'flowgger_amd' / 'host'}", "-o", str(exe2), str(Path(td) / "splitter_hop.cpp")], check=True)
        for name, raw in corpora(mib).items():
            dec = RFC5424Decoder()
            gib = len(raw) / (1 << 30)
            (Path(td) / "s.bin").write_bytes(raw)
            walk_ms = float(subprocess.run([str(exe), str(Path(td) / "s.bin")], capture_output=True, text=True, check=True).stdout)
            hop_ms = float(subprocess.run([str(exe2), str(Path(td) / "s.bin")], capture_output=True, text=True, check=True).stdout)
            d = torch.zeros((len(raw) + 31) // 16 * 16, dtype=torch.uint8, device="cuda")
            d[:len(raw)] = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
            d_raw = d[:len(raw)]
            d_packed, d_offs, d_starts, d_bad, n, consumed, stop = dec.frame_syslen_device(d_raw)
            cap = n + 16
            a = best_ms(lambda: dec.frame_syslen_device(d_raw, cap_frames=cap))
            total = int(d_offs[-1])
            d_pay = torch.zeros((total + 31) // 16 * 16, dtype=torch.uint8, device="cuda")
            d_pay[:total] = d_packed[:total]
            b = best_ms(lambda: dec.frame_device(d_pay[:total], L.FG_FRAME_LINE, cap_frames=cap))
            pin = pinned_copy(L, raw)
            st, off, nn, used = L.fg_tables(), C.c_void_p(), C.c_uint64(), C.c_uint64()

            def new_route():
                L.check(L.lib().fg_frame_decode_batch(dec._ctx, dec.fmt, L.FG_FRAME_SYSLEN, pin, len(raw), 1, C.byref(st), C.byref(off), C.byref(nn),
                                                      C.byref(used)), "fg_frame_decode_batch")

            new_route()
            d_new = wall_ms(new_route)
            path = L.lib().fg_last_host_path(dec._ctx)
            pay = d_packed[:total].cpu().numpy().tobytes()
            pin_pay = pinned_copy(L, pay)
            offs_np = d_offs.cpu().numpy().astype(np.uint64)
            pin_off = pinned_copy(L, offs_np.tobytes())

            def old_decode():
                L.check(L.lib().fg_decode_batch(dec._ctx, dec.fmt, pin_pay, total, pin_off, n, C.byref(st)), "fg_decode_batch")

            old_decode()
            d_old = wall_ms(old_decode)
            print(json.dumps({"corpus": name, "MiB": round(len(raw) / (1 << 20), 1), "frames": n, "path": path,
                              "a_frame_pack_ms_per_GiB": [round(x / gib, 3) for x in a], "b_line_framer_ms_per_GiB": [round(x / gib, 3) for x in b],
                              "c_splitter_hop_ms_per_GiB": round(hop_ms / gib, 2), "c2_host_walk_ms_per_GiB": round(walk_ms / gib, 2),
                              "d_new_ms_min_med_max": [round(x, 3) for x in d_new], "d_parent_decode_ms_min_med_max": [round(x, 3) for x in d_old],
                              "d_parent_route_ms_med": round(d_old[1] + hop_ms, 3)}), flush=True)
            for p in (pin, pin_pay, pin_off):
                L.lib().fg_free_pinned(p)


def main():
    args = sys.argv[1:]
    mib = int(args[args.index("--mib") + 1]) if "--mib" in args else 256
    if "--step" in args:
        step = args[args.index("--step") + 1]
        return step_check() if step == "check" else step_measure(mib)
    for step, limit in (("check", 120), ("measure", 420)):
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, __file__, "--step", step, "--mib", str(mib)])
        if r.returncode != 0:  # (a step that failed ends the probe: nothing more is started on the GPU)
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
