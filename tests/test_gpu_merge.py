"""-m gpu: the ordered device merge (fg_merge_tables_device -> fg_launch_merge_device: k_merge_rows, k_merge_block_sums, the scan
borrowed from the encoders, k_merge_entries) against the model of tests/merge_model.py, which tests/test_merge_model_cpu.py has
qualified against the host merge.  The merge moves rows and entries and never looks at them, so synthetic tables reach every path:
part counts 1 .. 8, empty parts, the edges of the 64-row blocks, rows of more than 64 entries, overflowed parts, unnamed and
out-of-range positions, the ent_cap guard, the src_part carved out of the scratch, the grid-stride loop and the second round of the
block scan.  Every synthetic case is bit-exact over the WHOLE output allocation (prefilled with 0xA5) and the whole src_part array: a
store outside what the merge owns fails the test.

A caller contract that is deliberately NOT exercised: an index that names one position TWICE.  Two lanes then write the columns of
one row concurrently; the row may end up with one part's ent_first under another part's tag, and the entry copy would read outside a
part's table.  That is undefined by contract (include/fg_hip.h: every position once) and an out-of-bounds read is nothing to provoke on real hardware.
Two rows of one part that share a SLICE are deterministic (the reads stay inside the part) and are what the ent_cap guard is run on.
"""
import ctypes as C

import numpy as np
import pytest

import merge_model as mm
from flowgger_amd import GelfDecoder, LTSVDecoder, RFC5424Decoder, shard, synth
from flowgger_amd import _lib as L
from flowgger_amd.tables import DeviceTables
from gpu_util import assert_same, device_path, rows_of_part

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dec():
    d = RFC5424Decoder()
    yield d
    d.close()


@pytest.fixture(scope="module")
def oracle():
    import oracle_binding

    return oracle_binding.Oracle()


def device_of(dec):
    import torch

    return torch.device("cuda", dec.device)


def upload_index(index, dev):
    """index[k] on the device; an empty part gets NO array (data_ptr() of an empty tensor is 0: a null pointer)"""
    import torch

    out = []
    for ix in index:
        if ix is None or len(ix) == 0:
            out.append(torch.empty(0, dtype=torch.int64, device=dev))
            assert out[-1].data_ptr() == 0
        else:
            out.append(torch.from_numpy(np.ascontiguousarray(ix).astype(np.int64)).to(dev))
    return out


def fresh_output(n, ent_cap, dev, spare=0):
    """(DeviceTables, src_part) prefilled with 0xA5; spare: entries of capacity allocated but not told to the merge"""
    import torch

    out = DeviceTables(n, ent_cap + spare, dev)
    out.buf.fill_(mm.FILL)
    if spare:
        out.ent_cap = ent_cap
        out.struct.ent_cap = ent_cap
    d_src = torch.full((max(n, 1),), mm.FILL, dtype=torch.uint8, device=dev)
    return out, d_src


def c_merge(dec, structs, index_ptrs, out_struct, d_src_ptr, g=None, ctx="own"):
    """the C entry itself (torch's current stream); returns its code"""
    import torch

    arr = (L.fg_tables * max(len(structs), 1))(*structs)
    ptrs = (C.c_void_p * max(len(index_ptrs), 1))(*index_ptrs)
    stream = torch.cuda.current_stream(device_of(dec)).cuda_stream
    return L.lib().fg_merge_tables_device(dec._ctx if ctx == "own" else ctx, arr, len(structs) if g is None else g, ptrs,
                                          C.byref(out_struct), d_src_ptr, C.c_void_p(stream))


def check_image(out, d_src, m, alloc_cap, base=None, src_base=None, what=""):
    got = out.buf.cpu().numpy()
    want = mm.expected_image(m, out.ent_cap, alloc_cap=alloc_cap, base=base)
    assert np.array_equal(got, want), f"{what}: {mm.first_difference(got, want, m.n, alloc_cap)}"
    if d_src is not None:
        gsrc = d_src.cpu().numpy()
        wsrc = mm.expected_src(m, len(gsrc), base=src_base)
        assert np.array_equal(gsrc, wsrc), f"{what}: src_part differs at {np.flatnonzero(gsrc != wsrc)[:8]}"
    return got


def run_case(dec, parts, index, spare=0, null_src=False, what=""):
    """upload, merge into a 0xA5 output, compare everything with the model; returns (out, d_src, model, image)"""
    import torch

    dev = device_of(dec)
    dparts = [mm.upload(p, dev) for p in parts]
    d_index = upload_index(index, dev)
    n, cap = sum(p.n for p in parts), sum(p.ent_cap for p in parts)
    out, d_src = fresh_output(n, cap, dev, spare)
    if null_src:
        rc = c_merge(dec, [p.struct for p in dparts], [int(i.data_ptr()) for i in d_index], out.struct, None)
        assert rc == L.FG_OK, rc
    else:
        out2, src2 = shard.merge_tables_device(dec, dparts, d_index, out=out, d_src=d_src)
        assert out2 is out and src2.numel() == n and (n == 0 or src2.data_ptr() == d_src.data_ptr())
    torch.cuda.synchronize(dev)
    m = mm.model(parts, index)
    img = check_image(out, None if null_src else d_src, m, cap + spare, what=what)
    assert not null_src or bool((d_src == mm.FILL).all().item())
    return out, d_src, m, img


def sweep_inputs(n, g, seed=0):
    tag, index = mm.deal(n, g, seed=4000 + 100 * g + n + seed, empty=(1,) if g >= 3 else ())
    parts = [mm.build_table(len(ix), seed=50 * g + k + seed, counts=mm.half_zero_1_70, gap_max=3, tail=k % 3) for k, ix in enumerate(index)]
    return parts, index


# ------------------------------------------------------------------------------------------------------ a. block edges x part counts
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 127, 128, 129, 193])
@pytest.mark.parametrize("g", [1, 2, 3, 8])
def test_block_edges_and_part_counts(dec, g, n):
    parts, index = sweep_inputs(n, g)
    assert g < 3 or (parts[1].n == 0 and len(index[1]) == 0)
    out, d_src, m, _ = run_case(dec, parts, index, what=f"g={g} n={n}")
    assert bool(m.named.all())


# ------------------------------------------------------------------------------------------------------------- b. hand-shaped blocks
@pytest.mark.parametrize("shape", ["empty_first_last", "one_row_200", "all_ones"])
def test_hand_shaped_blocks(dec, shape):
    counts = mm.block_shapes()[shape]
    tag, index = mm.deal(len(counts), 2, seed=31)
    parts = mm.parts_for_counts(counts, index, seed=32)
    out, d_src, m, _ = run_case(dec, parts, index, what=shape)
    assert np.array_equal(m.cols["ent_count"][:, 0], counts)


# ---------------------------------------------------------------------------------------------------------------------- c. empty input
@pytest.mark.parametrize("g", [1, 2, 8])
def test_all_parts_empty(dec, g):
    """out.n == 0: ent_used comes back 0, nothing else changes (src_part included)"""
    parts = [mm.build_table(0, seed=k, tail=3 * (k % 2)) for k in range(g)]  # (some with capacity and a counter, none with rows)
    out, d_src, m, img = run_case(dec, parts, [None] * g, what=f"empty g={g}")
    assert m.n == 0 and m.ent_used == 0
    assert int(np.count_nonzero(img != mm.FILL)) == 8


def test_tables_without_entry_capacity(dec):
    """parts of ent_cap 0 into an output of ent_cap 0: rows move, no entry is read or written"""
    tag, index = mm.deal(150, 3, seed=61)
    parts = [mm.build_table(len(ix), seed=62 + k, counts=np.zeros(len(ix), np.int64), gap_max=0) for k, ix in enumerate(index)]
    assert all(p.ent_cap == 0 for p in parts)
    out, d_src, m, _ = run_case(dec, parts, index, what="ent_cap 0")
    assert out.ent_cap == 0 and m.ent_used == 0


# ------------------------------------------------------------------------------------------------------------------ d. overflowed parts
@pytest.mark.parametrize("bad_is", [0, 1])
def test_overflowed_part_next_to_an_intact_one(dec, bad_is):
    """a part whose counter ran past its capacity: rows whose slice does not lie inside [0, ent_cap) own nothing in the merged table,
    every other row is merged as usual; ent_used = the sum of the kept counts"""
    bad, r0 = mm.overflow_part(seed=11, before=70, after=73)
    good = mm.build_table(150, seed=12)
    parts = [bad, good] if bad_is == 0 else [good, bad]
    tag, index = mm.deal_exact([p.n for p in parts], seed=13)
    out, d_src, m, _ = run_case(dec, parts, index, what=f"overflow in part {bad_is}")
    at = index[bad_is][r0:r0 + len(mm.OVERFLOW_ROWS)].astype(np.int64)
    assert m.cols["ent_count"][at, 0].tolist() == [c if ok else 0 for (f, c), ok in mm.OVERFLOW_ROWS]
    assert m.ent_used == int(m.cols["ent_count"].sum()) == int(good.a["ent_count"].sum()) + int(bad.a["ent_count"].sum()) - 15
    assert out.to_host().ent_used == m.ent_used


# --------------------------------------------------------------------------------------------------------------- e. reuse of the output
def test_second_merge_into_the_same_output(dec):
    """a framer merges batch after batch into the same memory: the second result is its model wherever the merge writes; entry slots
    behind the new ent_used still hold the first merge's values"""
    import torch

    dev = device_of(dec)
    n, g = 129, 3
    parts, index = sweep_inputs(n, g)
    out, d_src, m1, img1 = run_case(dec, parts, index, what="first merge")
    src1 = d_src.cpu().numpy()
    tag2, index2 = mm.deal(n, g, seed=77, empty=(0,))
    parts2 = [mm.build_table(len(ix), seed=78 + k, counts=mm.small_0_3, gap_max=1) for k, ix in enumerate(index2)]
    m2 = mm.model(parts2, index2)
    assert 0 < m2.ent_used < m1.ent_used and int((m2.cols["ent_count"] == 0).sum()) > 0
    assert bool(((m1.cols["ent_count"] > 0) & (m2.cols["ent_count"] == 0)).any())  # (a stale count that the merge must not scan)
    dparts2 = [mm.upload(p, dev) for p in parts2]
    out2, _ = shard.merge_tables_device(dec, dparts2, upload_index(index2, dev), out=out, d_src=d_src)
    torch.cuda.synchronize(dev)
    assert out2 is out
    check_image(out, d_src, m2, out.ent_cap, base=img1, src_base=src1, what="second merge")


# ------------------------------------------------------------------------------------------- f. unnamed and out-of-range positions
def test_unnamed_and_out_of_range_positions(dec):
    """an index >= out.n is skipped; the position nobody names has ent_count 0 and ent_first 0, contributes no entries, and its other
    row columns and its src_part byte keep what they held"""
    n = 130
    tag, index = mm.deal(n, 2, seed=21)
    parts = [mm.build_table(len(ix), seed=22 + k) for k, ix in enumerate(index)]
    whole = mm.model(parts, index)
    j = int(np.flatnonzero(parts[0].a["ent_count"][:parts[0].n] > 0)[3])  # (a row WITH entries: they must not reach the merged table)
    hole = int(index[0][j])
    index[0] = index[0].copy()
    index[0][j] = n + 5
    out, d_src, m, img = run_case(dec, parts, index, what="hole")
    assert not m.named[hole] and m.ent_used == whole.ent_used - int(whole.cols["ent_count"][hole, 0]) < whole.ent_used
    got = out.to_host()
    assert got.a["ent_count"][hole] == 0 and got.a["ent_first"][hole] == 0
    assert got.a["meta"][hole] == 0xA5A5A5A5 and d_src.cpu().numpy()[hole] == mm.FILL


# ------------------------------------------------------------------------------------------------------------------ g. the ent_cap guard
def test_entries_beyond_the_capacity_are_not_stored(dec):
    """two rows of one part share a slice, so the merged rows need more entries than out.ent_cap (by fewer than 64: the overflow
    falls inside one trip of the copy loop): ent_used reports it, entries [0, ent_cap) are the model's, nothing is stored at or behind
    ent_cap.  (The output is ALLOCATED with 256 entries more than the merge is told.)"""
    tag, index = mm.deal(100, 2, seed=91)
    parts = [mm.build_table(len(ix), seed=92 + k, gap_max=0) for k, ix in enumerate(index)]
    p = parts[0]
    cnt = p.a["ent_count"][:p.n]
    donor = int(np.flatnonzero((cnt >= 20) & (cnt < 64))[0])
    twin = int(np.flatnonzero(cnt == 0)[2])
    p.a["ent_first"][twin], p.a["ent_count"][twin] = p.a["ent_first"][donor], cnt[donor]
    cap = sum(q.ent_cap for q in parts)
    extra = int(cnt[donor])
    out, d_src, m, img = run_case(dec, parts, index, spare=256, what="ent_cap guard")
    assert out.ent_cap == cap and m.ent_used == cap + extra and 0 < extra < 64
    off, size = out.offs[L.TABLE_FIELDS.index("ent_val")]
    assert size == 8 * (cap + 256) and bool((img[off + 8 * cap: off + size] == mm.FILL).all())
    off, _ = out.offs[L.TABLE_FIELDS.index("ent_used")]
    assert int(img[off:off + 8].view(np.uint64)[0]) == cap + extra


# ------------------------------------------------------------------------------------------------- h. src_part carved out of the scratch
@pytest.mark.parametrize("n", [1, 64, 4097])
def test_null_src_part(dec, n):
    """d_src_part == NULL through the C entry: the part tags live behind the n / 64 + 2 block sums of the ctx's scratch"""
    parts, index = sweep_inputs(n, 2, seed=7)
    run_case(dec, parts, index, null_src=True, what=f"null src_part n={n}")


# ----------------------------------------------------------------------------------------------------------------------------- i. scale
def test_grid_stride_and_second_scan_round(dec):
    """part 0 has more rows than the capped grid of k_merge_rows covers in one pass (CUs x 16 blocks of 256), and the merged table
    more than 524 288 rows (8 192 block sums: a second round of k_block_scan).  Vectorised checks only."""
    import torch

    dev = device_of(dec)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    sizes = [cus * 4096 + 257, 1000]
    n = sum(sizes)
    assert n > 524_288
    tag, index = mm.deal_exact(sizes, seed=101)
    parts = [mm.build_table(sz, seed=102 + k, counts=lambda r, m_: r.integers(0, 3, m_), gap_max=1) for k, sz in enumerate(sizes)]
    dparts = [mm.upload(p, dev) for p in parts]
    cap = sum(p.ent_cap for p in parts)
    out, d_src = fresh_output(n, cap, dev)
    shard.merge_tables_device(dec, dparts, upload_index(index, dev), out=out, d_src=d_src)
    torch.cuda.synchronize(dev)
    got = out.to_host()
    assert np.array_equal(d_src.cpu().numpy(), tag)
    cnt = np.zeros(n, np.int64)
    src_first = np.zeros(n, np.int64)
    for k, (p, ix) in enumerate(zip(parts, index)):
        at = ix.astype(np.int64)
        for col in ("meta", "ts"):
            assert np.array_equal(got.a[col][at], p.a[col][:p.n]), (k, col)
        for col in mm.SPAN_COLS:
            assert np.array_equal(got.a[col].reshape(-1, 2)[at], p.a[col].reshape(-1, 2)[:p.n]), (k, col)
        cnt[at] = p.a["ent_count"][:p.n]
        src_first[at] = p.a["ent_first"][:p.n]
    assert np.array_equal(got.a["ent_count"][:n], cnt)
    dense = np.cumsum(cnt) - cnt
    assert np.array_equal(got.a["ent_first"][:n], np.where(cnt > 0, dense, 0))
    total = int(cnt.sum())
    assert got.ent_used == total
    # entry e of the merged table = entry (src_first - dense)[its row] + e of its row's part
    take = np.repeat(src_first - dense, cnt) + np.arange(total)
    part_of = np.repeat(tag, cnt)
    for col, w in mm.ENT_COLS:
        want = np.zeros((total, w), got.a[col].dtype)
        for k, p in enumerate(parts):
            sel = part_of == k
            want[sel] = p.a[col].reshape(-1, w)[take[sel]]
        assert np.array_equal(got.a[col][: total * w].reshape(-1, w), want), col
    # and nothing behind ent_used, nor in the padding of the largest column, was written
    off, size = out.offs[L.TABLE_FIELDS.index("ent_val")]
    assert bool((out.buf[off + 8 * total: (off + size + 255) // 256 * 256] == mm.FILL).all().item())


# ------------------------------------------------------------------------------------------------------------------- j. real decoders
def test_eight_sub_batches_of_one_decoder_equal_the_oracle_on_the_whole_batch(dec, oracle):
    """4 000 RFC5424 lines dealt into 8 tagged sub-batches, each decoded on its own and merged: the merged table serialises, with the
    WHOLE batch's bytes, to the Records the oracle decodes from the whole batch"""
    import torch

    dev = device_of(dec)
    lines = synth.rfc5424_lines(4000, cfg=4, sd=True)
    data, offsets = synth.pack(lines)
    tag, index = mm.deal(len(lines), 8, seed=0x5424)
    dparts = []
    for ix in index:
        d, o = synth.pack([lines[int(i)] for i in ix])
        tables, _, _ = device_path(dec, d, o)
        dparts.append(tables)
    out, d_src = shard.merge_tables_device(dec, dparts, upload_index(index, dev))
    torch.cuda.synchronize(dev)
    assert np.array_equal(d_src.cpu().numpy(), tag)
    blob, offs = out.to_host().serialize(dec.fmt, data, offsets, cfg=dec._cfg)
    oblob, ooffs = oracle.decode_batch(dec.fmt, data, offsets, None)
    assert_same(blob, offs, oblob, ooffs, lines)


def test_three_formats_equal_the_oracle_per_part(oracle):
    import torch

    sub = [synth.rfc5424_lines(700, cfg=4, sd=True), synth.ltsv_lines(690), synth.gelf_lines(710)]
    decs = (RFC5424Decoder(), LTSVDecoder(synth.LTSV_CONFIG), GelfDecoder())
    cfgs = (None, synth.LTSV_CONFIG, None)
    dev = device_of(decs[0])
    tag, index = mm.deal_exact([len(s) for s in sub], seed=0x3F)
    dparts, packs = [], []
    for d_, lines in zip(decs, sub):
        data, offsets = synth.pack(lines)
        tables, _, _ = device_path(d_, data, offsets)
        dparts.append(tables)
        packs.append((data, offsets, lines))
    out, d_src = shard.merge_tables_device(decs[0], dparts, upload_index(index, dev))
    torch.cuda.synchronize(dev)
    got = out.to_host()
    src = d_src.cpu().numpy()
    assert np.array_equal(src, tag)
    for k, (d_, cfg, ix) in enumerate(zip(decs, cfgs, index)):
        data, offsets, lines = packs[k]
        rows = ix.astype(np.int64)
        assert np.array_equal(np.flatnonzero(src == k), np.sort(rows))
        blob, offs = rows_of_part(got, rows).serialize(d_.fmt, data, offsets, cfg=d_._cfg)
        oblob, ooffs = oracle.decode_batch(d_.fmt, data, offsets, cfg)
        assert_same(blob, offs, oblob, ooffs, lines)
    for d_ in decs:
        d_.close()


# -------------------------------------------------------------------------------------------------------------------------- k. refusals
def test_bad_arguments_are_refused_before_anything_is_launched(dec):
    """every one of these is FG_ERR_ARG, and the output (table and src_part) is still all 0xA5 afterwards"""
    import torch

    dev = device_of(dec)
    tag, index = mm.deal(100, 2, seed=111)
    parts = [mm.build_table(len(ix), seed=112 + k) for k, ix in enumerate(index)]
    assert all(p.n > 0 and p.ent_cap > 0 for p in parts)
    dparts = [mm.upload(p, dev) for p in parts]
    d_index = upload_index(index, dev)
    n, cap = 100, sum(p.ent_cap for p in parts)
    out, d_src = fresh_output(n, cap, dev)
    ptrs = [int(i.data_ptr()) for i in d_index]
    src = int(d_src.data_ptr())

    def copy_of(st):
        c = L.fg_tables()
        C.memmove(C.byref(c), C.byref(st), C.sizeof(L.fg_tables))
        return c

    def structs():
        return [copy_of(p.struct) for p in dparts]

    cases = {}
    cases["g = 0"] = c_merge(dec, structs(), ptrs, out.struct, src, g=0)
    nine = [copy_of(dparts[k % 2].struct) for k in range(9)]
    cases["g = 9"] = c_merge(dec, nine, [ptrs[k % 2] for k in range(9)], out.struct, src, g=9)
    for name, (dn, dcap) in {"out.n too small": (-1, 0), "out.n too large": (1, 0), "out.ent_cap below the sum": (0, -1)}.items():
        o = copy_of(out.struct)
        o.n, o.ent_cap = n + dn, cap + dcap
        cases[name] = c_merge(dec, structs(), ptrs, o, src)
    for col in L.TABLE_FIELDS:
        o = copy_of(out.struct)
        setattr(o, col, None)
        cases[f"out.{col} NULL"] = c_merge(dec, structs(), ptrs, o, src)
    for col in ("ent_used", "meta", "full_msg", "ent_count", "ent_name"):
        for k in (0, 1):
            s = structs()
            setattr(s[k], col, None)
            cases[f"part {k}: {col} NULL"] = c_merge(dec, s, ptrs, out.struct, src)
    for k in (0, 1):
        p2 = list(ptrs)
        p2[k] = None
        cases[f"index[{k}] NULL"] = c_merge(dec, structs(), p2, out.struct, src)
    cases["ctx NULL"] = c_merge(dec, structs(), ptrs, out.struct, src, ctx=None)
    assert len(cases) == 2 + 3 + 15 + 10 + 2 + 1
    torch.cuda.synchronize(dev)
    assert {k: v for k, v in cases.items() if v != L.FG_ERR_ARG} == {}
    assert bool((out.buf == mm.FILL).all().item()) and bool((d_src == mm.FILL).all().item())
    # ... and the same arguments, untouched, are accepted
    assert c_merge(dec, structs(), ptrs, out.struct, src) == L.FG_OK
    torch.cuda.synchronize(dev)
    check_image(out, d_src, mm.model(parts, index), cap, what="after the refusals")
