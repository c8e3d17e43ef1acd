"""The segmented octet-counted framer restated: every segment of the buffer is walked as if it were the whole chunk (`walk` of
syslen_binding.py per segment, with the device parser's bound), and the frames come out in buffer order, packed (test infrastructure)."""
from __future__ import annotations

import numpy as np

from syslen_binding import valid_utf8, walk

MAX_PREFIX = 24  # FG_SYSLEN_MAX_PREFIX: the device parser's bound


def clamp(seg_starts, nbytes):
    """the starts as the kernels use them: non-decreasing, inside the buffer, the first 0 and the last nbytes"""
    n_segs = len(seg_starts) - 1
    c, run = [], 0
    for k, v in enumerate(seg_starts):
        run = 0 if k == 0 else nbytes if k >= n_segs else min(max(int(v), run), nbytes)
        c.append(run)
    return c


def model(buf: bytes, seg_starts, bound: int | None = MAX_PREFIX):
    """-> dict(n, packed, offsets [n + 1], starts [n], bad [n], payloads, seg_first [K + 1], seg_consumed [K], seg_stop [K])"""
    c = clamp(seg_starts, len(buf))
    starts, payloads, seg_first, seg_consumed, seg_stop = [], [], [0], [], []
    for k in range(len(c) - 1):
        seg = buf[c[k]:c[k + 1]]
        st, pl, ln, consumed, stop = walk(seg, bound)
        for s, p, n in zip(st, pl, ln):
            starts.append(c[k] + s)
            payloads.append(seg[s + p:s + p + n])
        seg_first.append(len(starts))
        seg_consumed.append(consumed)
        seg_stop.append(stop)
    return {"n": len(starts), "packed": b"".join(payloads), "payloads": payloads,
            "offsets": [0] + [int(x) for x in np.cumsum([len(p) for p in payloads], dtype=np.int64)], "starts": starts,
            "bad": [0 if valid_utf8(p) else 1 for p in payloads], "seg_first": seg_first, "seg_consumed": seg_consumed, "seg_stop": seg_stop}


def assert_equal(r, m):
    """a framer's result r (arrays cut to their valid lengths) against the model m"""
    assert r["n"] == m["n"]
    assert list(r["seg_first"]) == m["seg_first"]
    assert list(r["seg_consumed"]) == m["seg_consumed"]
    assert list(r["seg_stop"]) == m["seg_stop"]
    assert list(r["starts"]) == m["starts"]
    assert list(r["offsets"]) == m["offsets"]
    assert bytes(r["packed"][:len(m["packed"])]) == m["packed"]
    assert list(r["bad"]) == m["bad"]


def edge_boundaries(nbytes: int, tile: int = 4096):
    """segment starts (sorted, with repeats) that put boundaries where the tiles of the device logic meet: at 4096 j - 1, 4096 j and
    4096 j + 1, empty and one-byte segments, 40 segments inside tile 16, and none at all between tiles 8 and 15 (a segment that spans
    six tiles).  For nbytes >= 18 tiles."""
    assert nbytes >= 18 * tile
    cuts = [tile - 1, tile, tile + 1, 2 * tile - 1, 3 * tile, 4 * tile + 1, 5 * tile, 5 * tile, 5 * tile, 6 * tile + 7, 6 * tile + 8, 8 * tile + 1,
            15 * tile - 1]
    cuts += [16 * tile + 3 + 100 * i for i in range(40)]
    cuts += [17 * tile, 17 * tile + 1, 17 * tile + 1, 17 * tile + 2]
    return cuts


def with_boundaries(nbytes: int, *lists):
    """seg_starts (K + 1 entries, 0 first, nbytes last) from lists of cut positions; repeats stay (empty segments)"""
    return [0] + sorted(int(x) for ls in lists for x in ls if 0 < x < nbytes) + [nbytes]


def declining_stream():
    """test_gpu_syslen.py's: a message whose body is a long list of distinct numbers across a tile end -- every "1234 " is a candidate
    that leaves its tile somewhere else, more exits than the kernels track"""
    wrap = lambda msgs: b"".join(b"%d %s\n" % (len(m) + 1, m) for m in msgs)
    body = b" ".join(b"%d" % i for i in range(1000, 1900))
    return wrap([b"<13>1 2024-01-02T03:04:05Z h a 1 m - first", body] +
                [b"<13>1 2024-01-02T03:04:05Z h a 1 m - filler %d " % i + b"x" * 200 for i in range(40)])


def stream_with_a_frame_at(msgs, at: int):
    """the messages wrapped ("<len> <msg>\\n") with filler frames put in so that a frame starts exactly at byte `at`: a segment that starts
    there is a chain of its own, not a BAD_LEN at its first byte"""
    frame = lambda m: b"%d %s\n" % (len(m) + 1, m)
    out, n = [], 0
    for k, m in enumerate(msgs):
        f = frame(m)
        if n <= at < n + len(f) and n != at:
            gap = at - n
            fill = next((b"%d %s" % (a, b"f" * a) + (b"%d %s" % (b, b"g" * b) if b >= 0 else b"") for a in range(gap) for b in range(-1, gap)
                         if len(b"%d " % a) + a + (len(b"%d " % b) + b if b >= 0 else 0) == gap), None)
            assert fill is not None, gap
            out.append(fill)
            n += gap
        out.append(f)
        n += len(f)
    assert n > at
    return b"".join(out)
