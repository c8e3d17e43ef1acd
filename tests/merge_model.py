"""The ordered device merge (fg_merge_tables_device, csrc/fg_merge.hip) restated in plain numpy: a seeded builder of synthetic
tables, the merged table ROW BY ROW as include/fg_hip.h and the comments of fg_merge.hip define it, and the byte image a whole
DeviceTables.buf must hold afterwards.  No GPU and no torch at import time (upload() imports torch when it is called).

The merge moves table rows and entries; it never looks at what they mean.  Random columns therefore reach every path of the three
kernels (part counts, 64-row block edges, rows of many entries, overflowed parts, unnamed positions) at a few hundred rows, and a
comparison of the WHOLE output allocation with the image shows a store outside what the merge owns.

What the merge owns, and what the image holds:
  * a position some index[k][j] names: the eight copied columns of row j of part k, src_part = k, ent_count = the row's count if its
    slice lies inside [0, min(counter_k, ent_cap_k)), else 0, ent_first = the exclusive running sum of those counts in arrival
    order (0 where the count is 0);
  * a position NO index names: ent_count = 0 and ent_first = 0 (the launcher zeroes every count before the rows are placed, and the
    entry kernel rewrites ent_first of every position from its count); the eight copied columns and the src_part byte are not touched;
  * entry slots [0, min(ent_used, ent_cap)) of the four entry columns, ent_used = the sum of the kept counts (it may exceed ent_cap
    when the caller's indices break the contract; nothing is stored at or behind ent_cap);
  * the eight bytes of ent_used.
Every other byte of the allocation -- column padding, entry slots behind ent_used -- keeps its value.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np

from flowgger_amd import _lib as L
from flowgger_amd.tables import HostTables, _DT, layout

FILL = 0xA5
SPAN_COLS = ("hostname", "appname", "procid", "msgid", "msg", "full_msg")
COPIED_COLS = ("meta", "ts") + SPAN_COLS                 # with ent_first / ent_count: the ten fixed columns of a row
ENT_COLS = (("ent_name", 2), ("ent_val", 1), ("ent_type", 1), ("ent_flags", 1))  # (column, elements of its dtype per entry)
_WIDTH = {"meta": 1, "ts": 1, "ent_first": 1, "ent_count": 1, **{c: 2 for c in SPAN_COLS}}


# ---------------------------------------------------------------------------------------------------------------- count distributions
def half_zero_1_70(rng: np.random.Generator, m: int) -> np.ndarray:
    """half of the rows own nothing, the rest 1 .. 70 entries (more than 64: a second trip of the entry kernel's copy loop)"""
    c = rng.integers(1, 71, m)
    c[rng.random(m) < 0.5] = 0
    return c


def small_0_3(rng: np.random.Generator, m: int) -> np.ndarray:
    return rng.integers(0, 4, m)


# ------------------------------------------------------------------------------------------------------------------------- the builder
def build_table(m: int, seed: int, counts=half_zero_1_70, gap_max: int = 3, ent_cap: Optional[int] = None,
                counter: Optional[int] = None, place: Optional[Dict[int, tuple]] = None, tail: int = 0) -> HostTables:
    """A HostTables of m rows with random row columns.
    counts    callable(rng, m) or an array of m counts: ent_count per row.
    gap_max   0 .. gap_max unused slots in front of every slice (decoders strand reservations: ent_used exceeds the sum of ent_count);
              the gaps hold random entries too, so an entry copied from a gap differs from the one that belongs there.
    tail      unused slots behind the last slice.
    ent_cap   capacity of the entry columns (default: exactly what the slices and gaps take; 0 is allowed when nothing is placed).
    counter   the raw value of ent_used (default: what the slices and gaps take); larger than ent_cap = a table that overflowed.
    place     {row: (ent_first, ent_count)} written over the generated layout, for hand-placed rows (slices that straddle the
              capacity, rows that share a slice); nothing is checked.
    Every entry slot [0, ent_cap) is random in all four entry columns."""
    rng = np.random.default_rng(seed)
    a = {name: np.zeros(1, _DT[name]) for name in L.TABLE_FIELDS}
    mm = max(m, 1)
    a["meta"] = rng.integers(0, 1 << 32, mm, dtype=np.uint64).astype(np.uint32)
    a["ts"] = rng.random(mm) * 4.0e9 - 1.0e9
    for col in SPAN_COLS:
        a[col] = rng.integers(0, 1 << 32, 2 * mm, dtype=np.uint64).astype(np.uint32)
    cnt = np.asarray(counts(rng, m) if callable(counts) else counts, np.int64).reshape(-1)
    assert cnt.size == m
    gaps = rng.integers(0, gap_max + 1, m) if gap_max else np.zeros(m, np.int64)
    first = np.cumsum(gaps + cnt) - cnt
    laid = int((gaps + cnt).sum()) + tail
    if ent_cap is None:
        ent_cap = laid
    a["ent_count"] = np.zeros(mm, np.uint32)
    a["ent_first"] = np.zeros(mm, np.uint32)
    a["ent_count"][:m] = cnt
    a["ent_first"][:m] = np.where(cnt > 0, first, 0)  # (decoders leave 0 in rows without entries)
    for row, (f, c) in (place or {}).items():
        a["ent_first"][row], a["ent_count"][row] = f, c
    e = max(ent_cap, 1)
    a["ent_name"] = rng.integers(0, 1 << 32, 2 * e, dtype=np.uint64).astype(np.uint32)
    a["ent_val"] = rng.integers(0, 1 << 64, e, dtype=np.uint64)
    a["ent_type"] = rng.integers(0, 256, e).astype(np.uint8)
    a["ent_flags"] = rng.integers(0, 256, e).astype(np.uint8)
    a["ent_used"] = np.array([laid if counter is None else counter], np.uint64)
    return HostTables(m, ent_cap, a)


def deal(n: int, g: int, seed: int, empty: Sequence[int] = ()) -> tuple:
    """A random tag per arrival position: (tag uint8[n], [index_k uint64] for k < g); the parts in `empty` get no position."""
    rng = np.random.default_rng(seed)
    live = [k for k in range(g) if k not in empty]
    tag = np.asarray(live, np.uint8)[rng.integers(0, len(live), n)]
    return tag, [np.flatnonzero(tag == k).astype(np.uint64) for k in range(g)]


def deal_exact(sizes: Sequence[int], seed: int) -> tuple:
    """The same for parts of given sizes: (tag, [index_k]) with len(index_k) == sizes[k]."""
    rng = np.random.default_rng(seed)
    tag = rng.permutation(np.repeat(np.arange(len(sizes), dtype=np.uint8), sizes))
    return tag, [np.flatnonzero(tag == k).astype(np.uint64) for k in range(len(sizes))]


# --------------------------------------------------------------------------------------------------------------------------- the model
class Merged:
    """The merged table of the model: cols[name] for n rows (spans as [n, 2]), named[i] = some index names position i, src[i] = its
    part, ent[name] = the dense entry columns ([ent_used, width]), ent_used."""

    def __init__(self, n: int):
        self.n = n
        self.cols = {c: np.zeros((n, _WIDTH[c]), _DT[c]) for c in COPIED_COLS + ("ent_first", "ent_count")}
        self.named = np.zeros(n, bool)
        self.src = np.zeros(n, np.uint8)
        self.ent: Dict[str, np.ndarray] = {}
        self.ent_used = 0


def model(parts: Sequence[HostTables], index: Sequence[Optional[np.ndarray]]) -> Merged:
    n = sum(p.n for p in parts)
    m = Merged(n)
    origin: List[Optional[tuple]] = [None] * n  # (part, first, kept count) of the row at a position
    for k, p in enumerate(parts):
        used = min(p.ent_used, p.ent_cap)
        for j in range(p.n):
            i = int(index[k][j])
            if i >= n:
                continue  # an index outside the merged table is ignored
            for c in COPIED_COLS:
                m.cols[c][i] = p.a[c].reshape(-1, _WIDTH[c])[j]
            m.named[i] = True
            m.src[i] = k
            first, cnt = int(p.a["ent_first"][j]), int(p.a["ent_count"][j])
            if first + cnt > used:
                cnt = 0  # the slice does not lie inside the entries that exist: the row owns nothing in the merged table
            origin[i] = (k, first, cnt)
    pieces: Dict[str, list] = {c: [] for c, _ in ENT_COLS}
    running = 0
    for i in range(n):
        if origin[i] is None:
            continue  # (count 0, first 0: as Merged starts)
        k, first, cnt = origin[i]
        m.cols["ent_count"][i] = cnt
        m.cols["ent_first"][i] = running if cnt else 0
        if cnt:
            for c, w in ENT_COLS:
                pieces[c].append(parts[k].a[c].reshape(-1, w)[first:first + cnt])
            running += cnt
    for c, w in ENT_COLS:
        m.ent[c] = np.concatenate(pieces[c]) if pieces[c] else np.zeros((0, w), _DT[c])
    m.ent_used = running
    return m


def model_rows(m: Merged) -> list:
    """The per-row view of tests/test_shard_cpu.py::rows() with ent_type and ent_flags, of the model."""
    out = []
    for i in range(m.n):
        f, c = int(m.cols["ent_first"][i, 0]), int(m.cols["ent_count"][i, 0])
        out.append((int(m.cols["meta"][i, 0]), float(m.cols["ts"][i, 0]), tuple(tuple(int(x) for x in m.cols[s][i]) for s in SPAN_COLS),
                    tuple(int(v) for v in m.ent["ent_val"][f:f + c, 0]), tuple(tuple(int(x) for x in e) for e in m.ent["ent_name"][f:f + c]),
                    tuple(int(v) for v in m.ent["ent_type"][f:f + c, 0]), tuple(int(v) for v in m.ent["ent_flags"][f:f + c, 0])))
    return out


def table_rows(t: HostTables) -> list:
    """The same view of a HostTables (whatever its entry layout is: every row through its own ent_first)."""
    out = []
    sp = {c: t.a[c].reshape(-1, 2) for c in SPAN_COLS + ("ent_name",)}
    for i in range(t.n):
        f, c = int(t.a["ent_first"][i]), int(t.a["ent_count"][i])
        out.append((int(t.a["meta"][i]), float(t.a["ts"][i]), tuple(tuple(int(x) for x in sp[s][i]) for s in SPAN_COLS),
                    tuple(int(v) for v in t.a["ent_val"][f:f + c]), tuple(tuple(int(x) for x in e) for e in sp["ent_name"][f:f + c]),
                    tuple(int(v) for v in t.a["ent_type"][f:f + c]), tuple(int(v) for v in t.a["ent_flags"][f:f + c])))
    return out


# ----------------------------------------------------------------------------------------------------------------------- the byte image
def expected_image(m: Merged, ent_cap: int, alloc_cap: Optional[int] = None, base: Optional[np.ndarray] = None) -> np.ndarray:
    """What a DeviceTables(m.n, alloc_cap).buf holds after the merge into a table of ent_cap entries (alloc_cap defaults to ent_cap;
    a test may hand the merge a smaller capacity than it allocated).  base: the bytes before the merge (default: all FILL)."""
    alloc_cap = ent_cap if alloc_cap is None else alloc_cap
    offs, total = layout(m.n, alloc_cap)
    img = np.full(total, FILL, np.uint8) if base is None else np.array(base, np.uint8, copy=True)
    assert img.size == total
    every = np.ones(m.n, bool)
    for name, (off, size) in zip(L.TABLE_FIELDS, offs):
        dt = np.dtype(_DT[name])
        if name in m.cols:
            if m.n == 0:
                continue
            view = img[off:off + size].view(dt).reshape(m.n, -1)
            rows = every if name in ("ent_first", "ent_count") else m.named
            view[rows] = m.cols[name][rows]
        elif name in m.ent:
            keep = min(m.ent_used, ent_cap)
            w = m.ent[name].shape[1]
            img[off:off + keep * w * dt.itemsize].view(dt)[:] = m.ent[name][:keep].reshape(-1)
        else:
            assert name == "ent_used" and size == 8
            img[off:off + 8].view(np.uint64)[0] = m.ent_used
    return img


def expected_src(m: Merged, length: Optional[int] = None, base: Optional[np.ndarray] = None) -> np.ndarray:
    """The src_part array (at least one byte long, as shard.merge_tables_device allocates it) after the merge."""
    length = max(m.n, 1) if length is None else length
    img = np.full(length, FILL, np.uint8) if base is None else np.array(base, np.uint8, copy=True)
    img[:m.n][m.named] = m.src[m.named]
    return img


def first_difference(got: np.ndarray, want: np.ndarray, n: int, alloc_cap: int) -> str:
    """Where two images of one table differ first, by column and element (for an assertion message)."""
    if got.shape != want.shape:
        return f"sizes differ: {got.shape} vs {want.shape}"
    bad = np.flatnonzero(got != want)
    if bad.size == 0:
        return "equal"
    b = int(bad[0])
    offs, _ = layout(n, alloc_cap)
    for name, (off, size) in zip(L.TABLE_FIELDS, offs):
        if off <= b < off + (size + 255) // 256 * 256:
            item = np.dtype(_DT[name]).itemsize * (2 if name in SPAN_COLS + ("ent_name",) else 1)
            where = f"element {(b - off) // item}" if b < off + size else "the padding behind it"
            return (f"{bad.size} bytes differ, first at byte {b}: column {name}, {where}: "
                    f"got {got[b:b + 8].tobytes().hex()} want {want[b:b + 8].tobytes().hex()}")
    return f"{bad.size} bytes differ, first at byte {b}"


# ----------------------------------------------------------------------------------------------------------------------------- upload
def upload(t: HostTables, device, ent_cap: Optional[int] = None):
    """A fresh DeviceTables(t.n, ent_cap) (default: t.ent_cap) holding t: the row columns, the first min(t.ent_cap, ent_cap) entries
    and the RAW counter, one copy.  Bytes the table does not own are 0x5A."""
    import torch

    from flowgger_amd.tables import DeviceTables

    ent_cap = t.ent_cap if ent_cap is None else ent_cap
    d = DeviceTables(t.n, ent_cap, device)
    img = np.full(d.buf.numel(), 0x5A, np.uint8)
    for name, (off, size) in zip(L.TABLE_FIELDS, d.offs):
        if name == "ent_used":
            img[off:off + 8].view(np.uint64)[0] = t.a["ent_used"][0]
            continue
        src = t.a[name].view(np.uint8)
        if name in dict(ENT_COLS):
            size = min(size, min(t.ent_cap, ent_cap) * (size // ent_cap if ent_cap else 0))
        img[off:off + size] = src[:size]
    d.buf.copy_(torch.from_numpy(img))
    return d


# ------------------------------------------------------------------------------------------------- hand-written shapes (CPU and GPU tests)
# The overflow rule on known answers: a part of ent_cap 40 whose counter ran to 55.  (row: (ent_first, ent_count) -> kept?)
OVERFLOW_CAP, OVERFLOW_COUNTER = 40, 55
OVERFLOW_ROWS = [
    ((0, 5), True),     # an ordinary row
    ((30, 10), True),   # the slice ends exactly at ent_cap
    ((35, 10), False),  # it straddles ent_cap
    ((40, 3), False),   # it starts at ent_cap
    ((50, 2), False),   # it starts behind ent_cap (below the raw counter: the clamp of used_of() decides, not the counter)
    ((0, 0), True),     # a row flagged FG_ST_OVERFLOW, count 0 (what a decoder leaves when its reservation failed)
    ((10, 4), True),    # an ordinary row
]


def overflow_part(seed: int, before: int = 0, after: int = 0, counts=small_0_3) -> tuple:
    """The rows of OVERFLOW_ROWS behind `before` and in front of `after` ordinary rows whose slices lie in [14, 30) of the 40 slots.
    Returns (HostTables, first hand-written row)."""
    rng = np.random.default_rng(seed)
    m = before + len(OVERFLOW_ROWS) + after
    place = {before + r: fc for r, (fc, _) in enumerate(OVERFLOW_ROWS)}
    for j in list(range(before)) + list(range(before + len(OVERFLOW_ROWS), m)):
        c = int(counts(rng, 1)[0])
        place[j] = (int(rng.integers(14, 30 - c + 1)), c) if c else (0, 0)
    t = build_table(m, seed + 1, counts=np.zeros(m, np.int64), gap_max=0, ent_cap=OVERFLOW_CAP, counter=OVERFLOW_COUNTER, place=place)
    flagged = before + 5
    t.a["meta"][flagged] = (int(t.a["meta"][flagged]) & 0xFFFFFF00) | L.FG_ST_OVERFLOW
    return t, before


def block_shapes() -> dict:
    """Counts per arrival position for the hand-shaped 64-row blocks of the entry kernel."""
    first_block_empty = np.zeros(192, np.int64)
    first_block_empty[64] = 9       # in the second block only its FIRST row owns entries
    first_block_empty[191] = 11     # in the third block only its LAST row
    one_big = np.zeros(64, np.int64)
    one_big[17] = 200               # four trips of the copy loop, all for one row
    return {"empty_first_last": first_block_empty, "one_row_200": one_big, "all_ones": np.ones(192, np.int64)}


def parts_for_counts(counts: np.ndarray, index: Sequence[np.ndarray], seed: int, gap_max: int = 3) -> list:
    """Parts whose rows, once merged through `index`, carry counts[i] at arrival position i."""
    return [build_table(len(ix), seed + k, counts=counts[ix.astype(np.int64)], gap_max=gap_max) for k, ix in enumerate(index)]
