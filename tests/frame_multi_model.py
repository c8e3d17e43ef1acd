"""The segmented framer's contract as a model (test infrastructure, pure Python over tests/oracle_binding.py): every segment of the
buffer is handed to the oracle's framer as a stream of its own (`BufRead::lines()` / `split(0)` + str::from_utf8 per connection);
the unterminated tail of a segment that is not final becomes a CARRY slot; offsets are shifted by the segment's start."""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence

import numpy as np

LINE, NUL = 0, 1  # FG_FRAME_LINE, FG_FRAME_NUL
SLOT_FRAME, SLOT_BAD_UTF8, SLOT_CARRY = 0, 1, 2


def term_of(framing: int) -> bytes:
    return b"\n" if framing == LINE else b"\0"


def clamp_starts(seg_starts: Sequence[int], nbytes: int) -> List[int]:
    """what the kernels make of a list that does not tile: each value into [its predecessor, nbytes], the first 0, the last nbytes"""
    K = len(seg_starts) - 1
    out, run = [], 0
    for k, v in enumerate(seg_starts):
        run = 0 if k == 0 else nbytes if k >= K else min(max(int(v), run), nbytes)
        out.append(run)
    return out


class Slots(NamedTuple):
    offsets: np.ndarray       # n + 1
    kind: np.ndarray          # n
    seg_first: np.ndarray     # K + 1
    seg_consumed: np.ndarray  # K


def model(oracle, raw: bytes, seg_starts: Sequence[int], seg_final: Optional[Sequence[int]], framing: int) -> Slots:
    c = clamp_starts(seg_starts, len(raw))
    K = len(c) - 1
    t = term_of(framing)
    offsets, kind, first, consumed = [0], [], [], []
    for k in range(K):
        s, e = c[k], c[k + 1]
        seg = raw[s:e]
        first.append(len(kind))
        frames = oracle.frame(seg, "line" if framing == LINE else "nul") if seg else []
        for a, b, body, valid in frames:
            # the oracle's verdict is str::from_utf8 of exactly the slot's bytes (the terminators are ASCII)
            try:
                seg[a:b].decode("utf-8")
                ok = True
            except UnicodeDecodeError:
                ok = False
            assert ok == valid, (k, a, b)
            assert a + s == offsets[-1]
            offsets.append(b + s)
            kind.append(SLOT_FRAME if valid else SLOT_BAD_UTF8)
        carry = bool(seg) and not (seg_final is not None and seg_final[k]) and not seg.endswith(t)
        if carry:
            kind[-1] = SLOT_CARRY
            consumed.append(offsets[-2] - s)
        else:
            consumed.append(e - s)
        assert offsets[-1] == e or not seg
    first.append(len(kind))
    assert offsets[-1] == len(raw) or not raw
    return Slots(np.array(offsets, np.uint64), np.array(kind, np.uint8), np.array(first, np.uint64), np.array(consumed, np.uint64))
