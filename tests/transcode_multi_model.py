"""What fg_transcode_multi_batch adds to the segmented framers' models (frame_multi_model, syslen_multi_model, capnp_frame_multi_model):
the per-segment cut of octet-counted input, and the inputs on which it can go wrong (test infrastructure)."""
from __future__ import annotations

import numpy as np

FRAME, BAD_UTF8, CARRY, UNREACHED = 0, 1, 2, 3  # fg_slot_kind


def cut(bad, seg_first):
    """kinds of the frames of K segments from their UTF-8 verdicts (0 / 1): behind a segment's first 1 everything is UNREACHED"""
    kind = [int(b) for b in bad]
    for a, b in zip(seg_first[:-1], seg_first[1:]):
        hit = next((i for i in range(int(a), int(b)) if kind[i]), int(b))
        kind[hit + 1:int(b)] = [UNREACHED] * max(int(b) - hit - 1, 0)
    return kind


def _case(sizes, flagged):
    first = [0]
    for s in sizes:
        first.append(first[-1] + s)
    bad = [0] * first[-1]
    for i in flagged:
        bad[i] = 1
    return first, bad


def cut_hazards():
    """[(name, seg_first, bad)]: the inputs on which the cut can go wrong.  A workgroup is 64 frames."""
    cases = [
        ("empty segments before, between and behind the flagged one", *_case([0, 0, 5, 0, 0, 7, 0, 4, 0, 0], [8])),
        ("the flagged frame first in its segment", *_case([3, 5, 4], [3])),
        ("the flagged frame last in its segment: nothing to mark", *_case([3, 5, 4], [7])),
        ("flagged at index 0 and at index n - 1", *_case([4, 70, 3], [0, 76])),
        ("two flagged frames of one segment in different workgroups: the smaller wins", *_case([10, 300, 10], [250, 40])),
        ("a segment that spans several workgroups", *_case([5, 400, 5], [9])),
        ("n no multiple of 64", *_case([30, 37, 64], [31, 40, 129])),
        ("one segment", *_case([100], [63, 64])),
        ("one segment, nothing flagged", *_case([100], [])),
        ("flagged in every segment, every frame flagged in one", *_case([3, 3, 3], [1, 3, 4, 5, 8])),
        ("no frames", *_case([0, 0], [])),
        ("no segments", [0], []),
        ("3000 frames, flagged in three workgroups", *_case([7, 3000, 7], [7 + 70, 7 + 1000, 7 + 2900])),
    ]
    return cases


def random_cases(seed: int, count: int, n_max: int = 1000):
    """seeded (seg_first, bad) pairs with n <= n_max, runs of empty segments included"""
    rng = np.random.default_rng(seed)
    for _ in range(count):
        n = int(rng.integers(0, n_max + 1))
        k = int(rng.integers(1, 40))
        cuts = np.sort(rng.integers(0, n + 1, k - 1)) if k > 1 else np.zeros(0, np.int64)
        if k > 3 and rng.random() < 0.5:  # a run of empty segments
            j = int(rng.integers(0, k - 2))
            cuts[j:j + int(rng.integers(2, 6))] = cuts[j]
            cuts = np.sort(cuts)
        first = [0] + [int(x) for x in cuts] + [n]
        p = float(rng.choice([0.0, 0.002, 0.02, 0.3]))
        yield first, (rng.random(n) < p).astype(np.uint8).tolist()
