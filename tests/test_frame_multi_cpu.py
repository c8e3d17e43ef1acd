"""CPU: the boundary logic of the segmented framer (flowgger_amd/csrc/fg_frame_multi.hpp, compiled for the host by
tests/native/frame_multi_host.cpp) against the model of tests/frame_multi_model.py -- every segment framed by the oracle as a stream
of its own.  Each case runs the classic way (one lane per boundary over the whole buffer) and the one-pass way (every block applies
the bits that lie in it; blocks of 16 bytes put a block edge at every residue a boundary can have, blocks of 16 KiB are the kernel's),
lanes in both orders."""
import random

import numpy as np
import pytest

import oracle_binding
from frame_multi_binding import FrameMultiHost
from frame_multi_model import LINE, NUL, SLOT_BAD_UTF8, SLOT_CARRY, SLOT_FRAME, clamp_starts, model, term_of
from utf8_hazards import cuts, kinds

FRAMINGS = [LINE, NUL]
WAYS = [(0, False), (0, True), (16, False), (16, True), (16384, False)]


@pytest.fixture(scope="module")
def host():
    return FrameMultiHost()


@pytest.fixture(scope="module")
def oracle():
    return oracle_binding.Oracle()


def check(host, oracle, raw, starts, final, framing):
    want = model(oracle, raw, starts, final, framing)
    c = clamp_starts(starts, len(raw))
    t = term_of(framing)[0]
    new = sum(1 for p in sorted(set(c[1:-1])) if 0 < p < len(raw) and raw[p - 1] != t)
    for block, reverse in WAYS:
        got, gc, added = host.frame(raw, starts, final, framing, block, reverse)
        ctx = (raw, starts, final, framing, block, reverse)
        assert gc == c, ctx
        assert np.array_equal(got.offsets, want.offsets), ctx
        assert np.array_equal(got.kind, want.kind), (ctx, got.kind, want.kind)
        assert np.array_equal(got.seg_first, want.seg_first), ctx
        assert np.array_equal(got.seg_consumed, want.seg_consumed), ctx
        assert added == new, ctx  # (what the classic form adds to the block counts)
    return want


@pytest.mark.parametrize("framing", FRAMINGS)
def test_every_hazard_at_every_cut(host, oracle, framing):
    """the boundary falls `cut` bytes into the hazard; the hazard's slot starts right behind a terminator; the pad moves the boundary
    over every residue of a 16-byte block"""
    t = term_of(framing)
    n = 0
    for kind, cut in cuts(kinds(framing)):
        for pad in (0, 3, 9, 10, 11, 12, 13, 14):
            raw = b"a" * pad + t + b"pq" + kind.data + b"rs" + t
            p = pad + 3 + cut
            for final in ((0, 0), (1, 0), (0, 1), (1, 1)):
                check(host, oracle, raw, [0, p, len(raw)], final, framing)
                n += 1
            # ... and with nothing behind the hazard: the second segment is the buffer's tail
            raw2 = b"a" * pad + t + b"pq" + kind.data
            if 0 < p < len(raw2):
                check(host, oracle, raw2, [0, p, len(raw2)], (1, 1), framing)
                check(host, oracle, raw2, [0, p, len(raw2)], None, framing)
    assert n > 1000


@pytest.mark.parametrize("framing", FRAMINGS)
def test_short_and_empty_segments(host, oracle, framing):
    """segments of 0 .. 4 bytes in runs: the windows of neighbouring boundaries overlap"""
    t = term_of(framing)
    alphabet = [t, b"a", b"\xc3", b"\xa9", b"\xe2", b"\x82", b"\xac", b"\xf0", b"\x9f"]
    rng = random.Random(1234 + framing)
    seen = set()
    for _ in range(1500):
        K = rng.randint(2, 9)
        lens = [rng.choice((0, 1, 2, 3, 4)) for _ in range(K)]
        raw = b"".join(rng.choice(alphabet) for _ in range(sum(lens)))
        starts = [0]
        for ln in lens:
            starts.append(starts[-1] + ln)
        final = [rng.randint(0, 1) for _ in range(K)]
        want = check(host, oracle, raw, starts, final, framing)
        seen |= set(int(k) for k in want.kind)
    assert seen == {SLOT_FRAME, SLOT_BAD_UTF8, SLOT_CARRY}
    # every run of equal lengths, several segments long, of a sequence that a boundary cuts at every byte
    for ln in (1, 2, 3, 4):
        for seq in (b"\xf0\x9f\x98\x80", b"\xe2\x82\xac", b"\xc3\xa9", b"a\xc3" + t + b"\xa9"):
            raw = seq * 6
            starts = list(range(0, len(raw), ln)) + [len(raw)]
            starts = sorted(set(starts))
            for fin in (0, 1):
                check(host, oracle, raw, starts, [fin] * (len(starts) - 1), framing)


@pytest.mark.parametrize("framing", FRAMINGS)
def test_boundary_behind_a_delimiter_and_cr(host, oracle, framing):
    t = term_of(framing)
    raw = b"one" + t + b"two" + t + t + b"three"
    for p in range(1, len(raw)):
        for final in ((0, 0), (1, 1), (0, 1), (1, 0)):
            check(host, oracle, raw, [0, p, len(raw)], final, framing)
    # "\r" ends a final segment, a non-final one, and "\n" opens the next
    raw = b"abc\r" + b"\ndef\r" + b"ghi\r\n" + b"\n"
    starts = [0, 4, 9, 14, 15]
    for final in ((1, 1, 1, 1), (0, 0, 0, 0), (1, 0, 1, 0), (0, 1, 0, 1)):
        want = check(host, oracle, raw, starts, final, framing)
        if framing == LINE:
            assert int(want.kind[0]) == (SLOT_FRAME if final[0] else SLOT_CARRY)
            assert [int(x) for x in want.offsets[:3]] == [0, 4, 5]  # "abc\r" | "\n": the CR is its own connection's


@pytest.mark.parametrize("framing", FRAMINGS)
def test_a_list_that_does_not_tile_is_clamped(host, oracle, framing):
    t = term_of(framing)
    raw = (b"alpha" + t + b"be\xc3\xa9ta" + t + b"gam") * 3
    n = len(raw)
    for starts in ([5, 3, 2, 40, 7, n + 9], [0, n + 5, 4, n], [0, 10, 10, 9, 2 ** 63, 1], [3, n], [0, 0, 0, n, n], [7, 2 ** 64 - 1, 0]):
        c = clamp_starts(starts, n)
        assert c[0] == 0 and c[-1] == n and all(a <= b for a, b in zip(c, c[1:]))
        check(host, oracle, raw, starts, [1, 0] * (len(starts) // 2) + [0], framing)


def test_one_final_segment_is_the_plain_framer(host, oracle):
    for framing in FRAMINGS:
        t = term_of(framing)
        for raw in (b"x", t, b"abc" + t + b"d\xe2\x82", b"\x80" + t + b"ok" + t, b"a" * 40 + t + b"\xf0\x9f\x98"):
            want = check(host, oracle, raw, [0, len(raw)], [1], framing)
            fr = oracle.frame(raw, "line" if framing == LINE else "nul")
            assert [int(x) for x in want.offsets] == [0] + [e for _, e, _, _ in fr]
            assert [int(k) for k in want.kind] == [0 if v else 1 for _, _, _, v in fr]
