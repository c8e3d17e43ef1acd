"""The segmented Cap'n Proto framer restated: every segment of the buffer is framed as if it were the whole chunk (CapnpFramer.frame per
segment, its CapnpStreamError turned into a stop + consumed: `model` of capnp_frame_binding.py), and the slots come out in buffer order:
a FRAME slot per whole message, one CARRY slot for the bytes of a segment behind `consumed` (test infrastructure)."""
from __future__ import annotations

from capnp_frame_binding import model as one_model

FRAME, CARRY = 0, 2  # FG_SLOT_FRAME, FG_SLOT_CARRY


def clamp(seg_starts, nbytes):
    """the starts as the kernels use them: non-decreasing, inside the buffer, the first 0 and the last nbytes, every one but the last
    rounded down to a multiple of 8"""
    n_segs = len(seg_starts) - 1
    c, run = [], 0
    for k, v in enumerate(seg_starts):
        run = 0 if k == 0 else nbytes if k >= n_segs else min(max(int(v), run), nbytes)
        c.append(run if k >= n_segs else run & ~7)
    return c


def model(buf: bytes, seg_starts):
    """-> dict(n, offsets [n + 1], kind [n], seg_first [K + 1], seg_consumed [K], seg_stop [K])"""
    c = clamp(seg_starts, len(buf))
    offsets, kind, seg_first, seg_consumed, seg_stop = [], [], [0], [], []
    for k in range(len(c) - 1):
        offs, consumed, stop = one_model(buf[c[k]:c[k + 1]])
        offsets += [c[k] + o for o in offs[:-1]]
        kind += [FRAME] * (len(offs) - 1)
        if consumed < c[k + 1] - c[k]:
            offsets.append(c[k] + consumed)
            kind.append(CARRY)
        seg_first.append(len(offsets))
        seg_consumed.append(consumed)
        seg_stop.append(stop)
    return {"n": len(kind), "offsets": offsets + [len(buf)], "kind": kind, "seg_first": seg_first, "seg_consumed": seg_consumed, "seg_stop": seg_stop}


def assert_equal(r, m):
    """a framer's result r (arrays cut to their valid lengths) against the model m"""
    assert r["n"] == m["n"]
    assert list(r["seg_first"]) == m["seg_first"]
    assert list(r["seg_consumed"]) == m["seg_consumed"]
    assert list(r["seg_stop"]) == m["seg_stop"]
    assert list(r["offsets"]) == m["offsets"]
    assert list(r["kind"]) == m["kind"]


def with_boundaries(nbytes: int, *lists):
    """seg_starts (K + 1 entries, 0 first, nbytes last) from lists of cut positions, each rounded down to a multiple of 8; repeats stay
    (empty segments)"""
    return [0] + sorted(int(x) & ~7 for ls in lists for x in ls if 0 < x < nbytes) + [nbytes]
