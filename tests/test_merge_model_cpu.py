"""CPU: the model of the ordered device merge (tests/merge_model.py) is qualified here before tests/test_gpu_merge.py holds the kernels
against it: on inputs that follow the contract it must equal the HOST merge (fg_merge_tables, another implementation with another
entry layout) row for row; its overflow rule is checked on hand-written tables with known answers (the host merge refuses such
parts, so it cannot be the judge there); and the byte image is checked where it is easy to get wrong (holes, ent_used, padding)."""
import ctypes as C

import numpy as np
import pytest

import merge_model as mm
from flowgger_amd import _lib as L
from flowgger_amd import shard
from flowgger_amd.tables import layout


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 127, 128, 129, 200])
@pytest.mark.parametrize("g", [1, 2, 3, 5, 8])
def test_model_equals_the_host_merge(g, n):
    """every position once, no overflow, gaps between the slices: same rows, same entries per row, same src_part"""
    tag, index = mm.deal(n, g, seed=1000 * g + n, empty=(1,) if g > 2 else ())
    parts = [mm.build_table(len(ix), seed=7 * g + k, gap_max=3, tail=k % 3) for k, ix in enumerate(index)]
    assert g <= 2 or parts[1].n == 0
    assert any(p.ent_used > int(p.a["ent_count"][:p.n].sum()) for p in parts) or n < 3  # (the gaps are there)
    want, wsrc = shard.merge_tables(parts, index)
    got = mm.model(parts, index)
    assert got.n == want.n == n and bool(got.named.all())
    assert mm.model_rows(got) == mm.table_rows(want)
    assert np.array_equal(got.src, wsrc) and np.array_equal(got.src, tag)
    # dense: the model's entries are exactly the kept counts, the host merge carries the stranded slots along
    cnt = want.a["ent_count"][:n].astype(np.int64)
    assert got.ent_used == int(cnt.sum()) <= want.ent_used
    dense = np.cumsum(cnt) - cnt
    assert np.array_equal(got.cols["ent_first"][:, 0], np.where(cnt > 0, dense, 0))


def _host_merge_rc(parts, index, n_out, e_out):
    """fg_merge_tables through the C entry with every part's TRUE capacity (shard._part_array widens ent_cap to the counter)"""
    arr = (L.fg_tables * len(parts))()
    for k, p in enumerate(parts):
        C.memmove(C.byref(arr[k]), C.byref(p.struct), C.sizeof(L.fg_tables))
    ix = [np.ascontiguousarray(i, np.uint64) for i in index]
    ptrs = (C.c_void_p * len(ix))(*[a.ctypes.data for a in ix])
    out = shard._alloc_tables(n_out, e_out)
    return L.lib().fg_merge_tables(arr, len(parts), ptrs, C.byref(out.struct), None)


def test_overflow_rule_on_known_answers():
    part, r0 = mm.overflow_part(seed=3)
    assert r0 == 0 and part.n == len(mm.OVERFLOW_ROWS) and part.ent_cap == 40 and part.ent_used == 55
    index = [np.arange(part.n, dtype=np.uint64)]
    got = mm.model([part], index)
    assert got.cols["ent_count"][:, 0].tolist() == [5, 10, 0, 0, 0, 0, 4]
    assert got.cols["ent_first"][:, 0].tolist() == [0, 5, 0, 0, 0, 0, 15]
    assert got.ent_used == 19
    take = list(range(0, 5)) + list(range(30, 40)) + list(range(10, 14))
    for col, w in mm.ENT_COLS:
        assert np.array_equal(got.ent[col], part.a[col].reshape(-1, w)[take]), col
    # the dropped rows keep their eight columns (the flagged one its status) and their part tag
    assert np.array_equal(got.cols["meta"][:, 0], part.a["meta"][:part.n]) and int(got.cols["meta"][5, 0]) & 0xFF == L.FG_ST_OVERFLOW
    assert bool(got.named.all()) and not got.src.any()
    # the host merge refuses the part instead
    assert _host_merge_rc([part], index, part.n, 64) == L.FG_ERR_ARG
    # a counter BELOW the capacity bounds the slices just as well: used = min(counter, ent_cap)
    low = mm.build_table(3, seed=4, counts=np.zeros(3, np.int64), gap_max=0, ent_cap=40, counter=20, place={0: (16, 4), 1: (18, 4), 2: (20, 1)})
    got = mm.model([low], [np.arange(3, dtype=np.uint64)])
    assert got.cols["ent_count"][:, 0].tolist() == [4, 0, 0] and got.ent_used == 4
    assert np.array_equal(got.ent["ent_val"][:, 0], low.a["ent_val"][16:20])


def test_overflow_rule_among_ordinary_rows():
    """the shape the GPU test runs: the hand-written rows keep their answers among 150 ordinary rows of an overflowed part, next to
    an intact part"""
    bad, r0 = mm.overflow_part(seed=11, before=70, after=73)
    good = mm.build_table(150, seed=12)
    tag, index = mm.deal_exact([bad.n, good.n], seed=13)
    got = mm.model([bad, good], index)
    at = index[0][r0:r0 + len(mm.OVERFLOW_ROWS)].astype(np.int64)
    kept = [c if ok else 0 for (f, c), ok in mm.OVERFLOW_ROWS]
    assert got.cols["ent_count"][at, 0].tolist() == kept
    assert got.ent_used == int(got.cols["ent_count"].sum()) == int(good.a["ent_count"].sum()) + int(bad.a["ent_count"].sum()) - 10 - 3 - 2
    assert _host_merge_rc([bad, good], index, bad.n + good.n, 4096) == L.FG_ERR_ARG


def test_image_leaves_holes_and_padding_alone():
    n = 130
    tag, index = mm.deal(n, 2, seed=21)
    parts = [mm.build_table(len(ix), seed=22 + k) for k, ix in enumerate(index)]
    whole = mm.model(parts, index)
    hole = int(index[0][5])
    index[0] = index[0].copy()
    index[0][5] = n + 5
    m = mm.model(parts, index)
    assert not m.named[hole] and int(m.named.sum()) == n - 1
    assert m.ent_used == whole.ent_used - int(whole.cols["ent_count"][hole, 0])
    cap = sum(p.ent_cap for p in parts)
    img = mm.expected_image(m, cap)
    offs, total = layout(n, cap)
    assert img.size == total
    by = dict(zip(L.TABLE_FIELDS, offs))
    for col in mm.COPIED_COLS:
        off, size = by[col]
        w = size // n
        assert bool((img[off + hole * w: off + (hole + 1) * w] == mm.FILL).all()), col
        assert bytes(img[off + (hole + 1) * w: off + (hole + 2) * w]) == m.cols[col][hole + 1].tobytes(), col
        assert bool((img[off + size: (off + size + 255) // 256 * 256] == mm.FILL).all()), col  # the padding behind the column
    for col in ("ent_first", "ent_count"):
        off, size = by[col]
        assert img[off:off + size].view(np.uint32)[hole] == 0
    off, size = by["ent_used"]
    assert size == 8 and int(img[off:off + 8].view(np.uint64)[0]) == m.ent_used
    assert bool((img[off + 8:] == mm.FILL).all())
    off, size = by["ent_val"]
    assert np.array_equal(img[off:off + 8 * m.ent_used].view(np.uint64), m.ent["ent_val"][:, 0])
    assert bool((img[off + 8 * m.ent_used: off + size] == mm.FILL).all())  # the slots behind ent_used
    src = mm.expected_src(m)
    assert src[hole] == mm.FILL and np.array_equal(np.delete(src, hole), np.delete(tag, hole))
    # a smaller capacity than the allocation: nothing at or behind it
    img2 = mm.expected_image(m, m.ent_used - 10, alloc_cap=cap)
    assert np.array_equal(img2[off:off + 8 * (m.ent_used - 10)], img[off:off + 8 * (m.ent_used - 10)])
    assert bool((img2[off + 8 * (m.ent_used - 10): off + size] == mm.FILL).all())
    assert int(img2[by["ent_used"][0]:][:8].view(np.uint64)[0]) == m.ent_used
    # an empty merge owns the counter alone
    e = mm.expected_image(mm.model([mm.build_table(0, 1), mm.build_table(0, 2)], [None, None]), 0)
    o = layout(0, 0)[0][-1][0]
    assert int(e[o:o + 8].view(np.uint64)[0]) == 0 and bool((np.delete(e, np.arange(o, o + 8)) == mm.FILL).all())


def test_hand_shaped_blocks_are_what_they_claim():
    shapes = mm.block_shapes()
    c = shapes["empty_first_last"]
    assert c[:64].sum() == 0 and np.flatnonzero(c[64:128]).tolist() == [0] and np.flatnonzero(c[128:]).tolist() == [63]
    assert shapes["one_row_200"].size == 64 and shapes["one_row_200"].max() == 200 and np.count_nonzero(shapes["one_row_200"]) == 1
    for name, counts in shapes.items():
        tag, index = mm.deal(len(counts), 2, seed=31)
        m = mm.model(mm.parts_for_counts(counts, index, seed=32), index)
        assert np.array_equal(m.cols["ent_count"][:, 0], counts), name
        assert m.ent_used == int(counts.sum())
