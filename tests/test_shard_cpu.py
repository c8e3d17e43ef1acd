"""CPU: the N>1 path -- byte-balanced sharding, ordered host gather (single process and
world_size-2 torch.distributed over gloo), and config 5's ordered merge of format sub-batches.
A deterministic numpy stand-in produces table rows, so the plumbing is tested without a GPU."""
import os

import numpy as np
import pytest

from flowgger_amd import _lib as L
from flowgger_amd import shard, synth
from flowgger_amd.tables import HostTables, _DT


def fake_decode(data, offsets, k=0):
    """Content-derived table rows (shard-independent by construction)."""
    offsets = offsets.astype(np.int64)
    n = len(offsets) - 1
    lens = np.diff(offsets)
    first = np.array([data[offsets[i]] if lens[i] else 0 for i in range(n)], np.int64)
    cnt = (lens % 3).astype(np.uint32)
    used = int(cnt.sum())
    a = {name: np.zeros(1, _DT[name]) for name in L.TABLE_FIELDS}
    a["meta"] = ((first << 8) | (lens % 251)).astype(np.uint32)
    a["ts"] = lens.astype(np.float64) * 0.5
    for j, col in enumerate(("hostname", "appname", "procid", "msgid", "msg", "full_msg")):
        a[col] = np.stack([np.full(n, j, np.uint32), lens.astype(np.uint32)], 1).reshape(-1)
    a["ent_count"] = cnt
    a["ent_first"] = (np.cumsum(cnt) - cnt).astype(np.uint32)
    vals, names = [], []
    for i in range(n):
        for e in range(int(cnt[i])):
            vals.append(int(first[i]) * 1000 + e)
            names.append((e, int(lens[i])))
    a["ent_val"] = np.array(vals or [0], np.uint64)
    a["ent_name"] = np.array(names or [(0, 0)], np.uint32).reshape(-1)
    a["ent_type"] = np.zeros(max(used, 1), np.uint8)
    a["ent_flags"] = np.zeros(max(used, 1), np.uint8)
    a["ent_used"] = np.array([used], np.uint64)
    return HostTables(n, used, a)


def rows(t: HostTables):
    out = []
    sp = {c: t.a[c].reshape(-1, 2) for c in ("hostname", "appname", "procid", "msgid", "msg", "full_msg", "ent_name")}
    for i in range(t.n):
        f, c = int(t.a["ent_first"][i]), int(t.a["ent_count"][i])
        out.append((int(t.a["meta"][i]), float(t.a["ts"][i]), tuple(tuple(sp[k][i]) for k in list(sp)[:6]),
                    tuple(int(v) for v in t.a["ent_val"][f:f + c]), tuple(tuple(x) for x in sp["ent_name"][f:f + c])))
    return out


@pytest.fixture(scope="module")
def corpus():
    lines = synth.rfc5424_lines(3000, cfg=5, sd=True, long_tail=True)
    return synth.pack(lines)


@pytest.mark.parametrize("g", [1, 2, 3, 8])
def test_sharded_equals_unsharded(corpus, g):
    data, offsets = corpus
    full = fake_decode(data, offsets)
    got = shard.decode_sharded(fake_decode, data, offsets, g)
    assert got.n == full.n and got.ent_used == full.ent_used
    assert rows(got) == rows(full)
    starts = shard.shard_plan(offsets, g)
    per = np.diff(offsets[starts].astype(np.int64))
    assert per.sum() == int(offsets[-1]) and per.max() - per.min() <= 2 * 8192


def _worker(rank, world, port, tmp):
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        lines = synth.rfc5424_lines(3000, cfg=5, sd=True, long_tail=True)
        data, offsets = synth.pack(lines)
        got = shard.decode_distributed(fake_decode, data, offsets, dst=0)
        if rank == 0:
            assert rows(got) == rows(fake_decode(data, offsets))
            open(os.path.join(tmp, "ok"), "w").write("1")
        else:
            assert got is None
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_distributed_gather_gloo_world2(tmp_path):
    import torch.multiprocessing as mp

    port = 29500 + os.getpid() % 2000
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    assert (tmp_path / "ok").exists()


@pytest.mark.parametrize("workload,world", [("cfg2", 2), ("cfg5mix", 2), ("cfg4", 8), ("cfg5mix", 8)])
def test_bench_dry_run_n_ranks(workload, world):
    """bench.py --dry-run-backend gloo --gpus N: the N-rank control flow of the bench (self-launch under torch.distributed.run,
    process group, every barrier / reduction / gather, cfg5mix's merge + rank gather through the C ABI) on the CPU -- a hang in a
    collective shows up here, not on the first 8-GPU box.  Round 6: also at EIGHT ranks, for
    the two configurations BASELINE runs on eight GPUs -- configs[3] (`cfg4`, sharded) and configs[4] (`cfg5mix`, with its ordered gather)."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", str(world), "--dry-run-backend", "gloo", "--workload", workload,
                        "--steps", "3", "--warmup", "1", "--full"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["dry_run"] is True and line["n_gpus"] == world and line["ranks"]["n"] == world and line["calibration_ranks"] == world
    if workload == "cfg5mix":
        assert line["gather"]["ranks_rows"] == sum(1000 + 10 * r for r in range(world)) and len(line["gather"]["all_ranks_gather_ms"]) == world
    elif workload == "cfg2":
        assert line["e2e_legs"] == ["decode_batch", "frame_decode_batch", "frame_decode_batch_two_step", "link_peak", "transcode_batch"]
    else:
        assert line["e2e_legs"] == ["decode_batch", "frame_decode_batch", "frame_decode_batch_two_step", "link_peak"]


def test_ordered_merge_of_format_sub_batches(oracle):
    """Config 5: RFC5424 and LTSV lines interleaved; each sub-batch is decoded on its own and the
    results are re-interleaved by original index."""
    a = synth.rfc5424_lines(300, cfg=5, long_tail=True)
    b = synth.ltsv_lines(200, long_tail=True)
    rng = np.random.default_rng(5)
    tag = rng.permutation(np.array([0] * len(a) + [1] * len(b)))
    ia, ib = np.nonzero(tag == 0)[0], np.nonzero(tag == 1)[0]
    da, oa = synth.pack(a)
    db, ob = synth.pack(b)
    ba, offa = oracle.decode_batch(0, da, oa)
    bb, offb = oracle.decode_batch(1, db, ob, synth.LTSV_CONFIG)
    blob, offs = shard.ordered_merge([(ia, ba, offa), (ib, bb, offb)])
    it = {0: iter(a), 1: iter(b)}
    for i, t in enumerate(tag):
        line = next(it[int(t)])
        want = oracle.decode(int(t), line, synth.LTSV_CONFIG if t else None)
        assert blob[int(offs[i]):int(offs[i + 1])].tobytes() == want


def test_merge_tables_restores_original_positions(corpus):
    """fg_merge_tables: two sub-batches split off by a per-line tag go back to their original rows; entries follow."""
    data, offsets = corpus
    n = len(offsets) - 1
    full = fake_decode(data, offsets)
    rng = np.random.default_rng(55)
    tag = rng.integers(0, 2, n)
    parts, index = [], []
    for k in (0, 1):
        ix = np.nonzero(tag == k)[0]
        lines = [data[int(offsets[i]):int(offsets[i + 1])].tobytes() for i in ix]
        d, o = synth.pack(lines)
        parts.append(fake_decode(d, o))
        index.append(ix)
    got, src = shard.merge_tables(parts, index)
    assert rows(got) == rows(full)
    assert np.array_equal(src, tag.astype(np.uint8))
    # a position used twice / out of range / decreasing is refused, not silently merged
    bad = [index[0].copy(), index[1].copy()]
    bad[1][0] = bad[0][0]
    with pytest.raises(L.FgError):
        shard.merge_tables(parts, bad)


def test_gather_and_merge_at_scale_take_milliseconds():
    """1 M rows through the C-ABI gather / merge: a few memory passes, no per-line Python (the round-1 Python loop took
    seconds per 100 K lines)."""
    import time

    n = 1_000_000
    rng = np.random.default_rng(9)
    lens = rng.integers(64, 512, n)

    def table(m, seed):
        r = np.random.default_rng(seed)
        a = {name: np.zeros(1, _DT[name]) for name in L.TABLE_FIELDS}
        a["meta"] = r.integers(0, 1 << 31, m).astype(np.uint32)
        a["ts"] = r.random(m)
        for col in ("hostname", "appname", "procid", "msgid", "msg", "full_msg"):
            a[col] = r.integers(0, 1 << 20, 2 * m).astype(np.uint32)
        cnt = r.integers(0, 4, m).astype(np.uint32)
        used = int(cnt.sum())
        a["ent_count"] = cnt
        a["ent_first"] = (np.cumsum(cnt) - cnt).astype(np.uint32)
        a["ent_val"] = r.integers(0, 1 << 60, max(used, 1)).astype(np.uint64)
        a["ent_name"] = r.integers(0, 1 << 20, 2 * max(used, 1)).astype(np.uint32)
        a["ent_type"] = np.zeros(max(used, 1), np.uint8)
        a["ent_flags"] = np.zeros(max(used, 1), np.uint8)
        a["ent_used"] = np.array([used], np.uint64)
        return HostTables(m, used, a)

    parts = [table(n // 8, s) for s in range(8)]
    t0 = time.perf_counter()
    got = shard.concat_tables(parts)
    dt_gather = time.perf_counter() - t0
    assert got.n == n and got.ent_used == sum(p.ent_used for p in parts)
    k = 5
    assert np.array_equal(got.a["meta"][k * (n // 8):(k + 1) * (n // 8)], parts[k].a["meta"][: n // 8])
    base = sum(p.ent_used for p in parts[:k])
    nz = np.nonzero(parts[k].a["ent_count"])[0][:100]
    assert np.array_equal(got.a["ent_first"][k * (n // 8) + nz], parts[k].a["ent_first"][nz] + base)
    # config 5 shape: two tagged halves, byte records of ~300 B
    tag = rng.integers(0, 2, n)
    recs = []
    for t in (0, 1):
        ix = np.nonzero(tag == t)[0]
        offs = np.zeros(len(ix) + 1, np.uint64)
        offs[1:] = np.cumsum(lens[ix])
        recs.append((ix, rng.integers(0, 255, int(offs[-1]), dtype=np.uint8), offs))
    t0 = time.perf_counter()
    blob, out_offs = shard.ordered_merge(recs)
    dt_merge = time.perf_counter() - t0
    assert np.array_equal(np.diff(out_offs.astype(np.int64)), lens)
    for t in (0, 1):
        ix, b, o = recs[t]
        for j in (0, 1, len(ix) // 2, len(ix) - 1):
            i = int(ix[j])
            assert np.array_equal(blob[int(out_offs[i]):int(out_offs[i + 1])], b[int(o[j]):int(o[j + 1])])
    print(f"gather 1M rows: {dt_gather * 1e3:.1f} ms; ordered merge 1M records ({len(blob) / 1e6:.0f} MB): {dt_merge * 1e3:.1f} ms")
    assert dt_gather < 2.0 and dt_merge < 5.0


def test_gather_and_merge_refuse_partially_filled_tables(corpus):
    """a C / Rust caller that leaves a column of `out` (or a blob pointer) NULL gets FG_ERR_ARG, not a null dereference."""
    import ctypes as C

    data, offsets = corpus
    part = fake_decode(data, offsets)
    assert part.ent_used > 0
    arr = shard._part_array([part])
    lib = L.lib()
    ix = np.arange(part.n, dtype=np.uint64)
    ptrs = (C.c_void_p * 1)(ix.ctypes.data)
    for hole in ("hostname", "full_msg", "ent_name", "ent_val", "ent_type", "ent_flags", "ent_count", "ent_used"):
        out = shard._alloc_tables(part.n, part.ent_used)
        setattr(out.struct, hole, None)
        assert lib.fg_gather_tables(arr, 1, C.byref(out.struct)) == L.FG_ERR_ARG, hole
        assert lib.fg_merge_tables(arr, 1, ptrs, C.byref(out.struct), None) == L.FG_ERR_ARG, hole
    # fg_ordered_merge: records without a blob
    m = np.array([2], np.uint64)
    offs = np.array([0, 3, 5], np.uint64)
    idx = np.array([0, 1], np.uint64)
    out_offs = np.zeros(3, np.uint64)
    vp = C.c_void_p
    rc = lib.fg_ordered_merge(1, m.ctypes.data, (vp * 1)(idx.ctypes.data), (vp * 1)(None), (vp * 1)(offs.ctypes.data), None, 0,
                              out_offs.ctypes.data)
    assert rc == L.FG_ERR_ARG


def test_mixed_cfg5_stream_and_merge_into_reused_buffers():
    """synth.mixed_cfg5 (BASELINE configs[4]): every arrival position belongs to exactly one sub-batch; fg_merge_tables into the
    buffers of an earlier call gives the same table."""
    tag, (la, ia), (lb, ib) = synth.mixed_cfg5(4000)
    assert len(la) == len(ia) and len(lb) == len(ib) and len(la) + len(lb) == 4000
    assert np.array_equal(np.sort(np.concatenate([ia, ib])), np.arange(4000, dtype=np.uint64))
    assert np.array_equal(tag[ia.astype(np.int64)], np.zeros(len(ia), np.uint8)) and bool((tag[ib.astype(np.int64)] == 1).all())
    assert la[0].startswith(b"<") and b"\t" in lb[0]
    parts = [fake_decode(*synth.pack(la)), fake_decode(*synth.pack(lb))]
    first, src = shard.merge_tables(parts, [ia, ib])
    want = rows(first)
    again, src2 = shard.merge_tables(parts, [ia, ib], out=first, src=src)
    assert again is first and rows(again) == want and np.array_equal(src2, tag)


def test_cpu_baseline_threads_are_persistent(oracle):
    """The CPU-baseline leg (oracle/fg_oracle.cpp fgo_bench_timed; VERDICT r2: the all-core figure was thread creation): with the
    threads parked before the clock starts, N threads do close to N times the work of one.  (Lenient: the box may be busy.)"""
    cores = min(len(os.sched_getaffinity(0)), 8)
    if cores < 2:
        pytest.skip("one core")
    data, offsets = synth.pack(synth.rfc5424_lines(20_000, cfg=2))
    s1, l1 = oracle.bench_timed(0, data, offsets, 1, 0.5)
    sn, ln = oracle.bench_timed(0, data, offsets, cores, 0.5)
    assert 0.45 < s1 < 1.5 and 0.45 < sn < 1.5
    eff = (ln / sn) / (l1 / s1) / cores
    assert eff > 0.35, eff
