"""GPU: the sparse window of the RFC5424 kernel for short lines (fg_pipeline.hpp persistent_loop<..., SPARSE>, fg_sparse_need.hpp).

Under force_sparse a wave fetches only the 16-byte chunks that hold the first H bytes or the last bytes of a line; the decoder makes a
row from those alone when no other byte can change it and decodes every other line again, whole.  A wave that handed back more than a
handful of lines stages dense until a group holds none.  Whatever the path, the rows are the oracle's: every case below is compared
with the oracle's canonical Records byte for byte, as tests/test_gpu_headline_loop.py does -- at one wave per CU and chunks of 16
lines (every wave goes round the loop and prefetches), with the default tile and with a 2 KiB tile (groups cut by bytes).

The hand-made lines of a case sit in a batch of filler lines twice: SPREAD, a few to the group (the wave stays sparse and hands them
back one by one), and PACKED, back to back (their groups hand back more than the handful: the groups behind them are staged dense,
and the filler behind those takes the wave back to sparse)."""
import re
from pathlib import Path

import numpy as np
import pytest

import test_gpu_headline_loop as hl
from flowgger_amd import RFC5424Decoder, synth
from golden.reference_vectors import RFC5424

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
H = int(re.search(r"kSparseHead\s*=\s*(\d+)", (ROOT / "flowgger_amd/csrc/fg_sparse_need.hpp").read_text()).group(1))
KNOBS = [{"waves_per_cu": 1, "chunk_lines": 16}, {"waves_per_cu": 1, "chunk_lines": 16, "tile_cap": 2048}]
KNOB_IDS = ["tile=default", "tile=2048"]
N_FILL = 9000  # lines of filler: with 16-line chunks at one wave per CU that is two chunks per wave and more (fg_plan_policy.hpp)
TS = b"2015-08-05T15:53:45Z"
BODY = b"the quick brown fox jumps over the lazy dog " * 4  # 176 bytes


def line(host=b"h", tail=b"- " + BODY, ts=TS):
    return b"<13>1 " + ts + b" " + host + b" app 4242 ID47 " + tail


def header_end(ln: bytes) -> int:
    """index behind the three bytes the cheap trim test reads: part 7 starts behind the sixth space"""
    pos = -1
    for _ in range(6):
        pos = ln.index(b" ", pos + 1)
    return pos + 1 + 3


def head_boundary_lines():
    """(b) the header, with the three bytes behind it, ends at every position from H - 8 to H + 8; one header of 140 bytes"""
    out = []
    base = header_end(line(host=b""))
    for end in list(range(H - 8, H + 9)) + [140]:
        ln = line(host=b"n" * (end - base))
        assert header_end(ln) == end and len(ln) > H + 20
        out.append(ln)
        out.append(line(host=b"n" * (end - base), tail=b"-  " + BODY))  # ... and a trim the cheap test does not settle, at the edge
    return out


def length_lines():
    """(c) every line length from 0 to H + 20: a valid line cut short, and a valid line of exactly that length"""
    full = line(host=b"host.example.org")
    out = [full[:k] for k in range(0, H + 21)]
    short = line(tail=b"- ")
    out += [short + b"m" * (k - len(short)) for k in range(len(short) + 1, H + 21)]
    return out


def trim_lines():
    """(e) both trim points: ASCII blanks, tabs, U+0085, U+2003, a run of blanks that reaches past H, a body of only whitespace"""
    nel, em = "\u0085".encode(), "\u2003".encode()
    out = []
    for ws in (b" ", b"   ", b"\t", b" \t ", nel, em, nel + em + b" ", b" " * (H + 30), b"\t" * H):
        out.append(line(tail=b"- " + ws + BODY))           # behind the '-'
        out.append(line(tail=b"-" + ws + BODY))
        out.append(line(tail=b"- " + BODY + ws))           # at the end of the line
        out.append(line(tail=b"- " + ws + BODY + ws))
        out.append(line(tail=b"- " + ws))                  # a body of only whitespace
        out.append(line(tail=b"-" + ws))
        out.append(line(host=b"n" * 60, tail=b"- " + ws + BODY + ws))  # ... with the header's end near H
    dash, e_acute = "\u2014".encode(), "\u00e9".encode()  # not whitespace: E2 80 94 shares two bytes with U+2003, C3 A9 is a two-byte char
    out.append(line(tail=b"- " + BODY + e_acute))
    out.append(line(tail=b"- " + BODY + dash))
    out.append(line(tail=b"- " + dash + BODY))
    out.append(line(tail=b"-" + e_acute + BODY + b" " + dash))
    return out


def sd_and_garbage_lines():
    """(f) short structured data and garbage where part 7 starts"""
    out = []
    for k in range(24):
        out.append(line(tail=b'[id%d a="b" c="d\\"e"] ' % k + BODY[: 40 + k]))
        out.append(line(tail=b'[x@1 k="v"][y@2 k2="v2"] m'))
        out.append(line(tail=b"x " + BODY))
        out.append(line(tail=b'[broken a="b" ' + BODY))
        out.append(line(tail=b"[a] " + BODY + b" "))
    return out


_fill = None


def filler():
    global _fill
    if _fill is None:
        _fill = synth.rfc5424_lines(N_FILL, cfg=2)  # (one line in a hundred is an invalid one)
    return _fill


def spread(special):
    """the special lines a few to the group: one every (N_FILL // len) filler lines, at least every ninth line"""
    fill = filler()
    step = max(9, N_FILL // max(len(special), 1))
    out, k = [], 0
    for i, ln in enumerate(fill):
        out.append(ln)
        if i % step == step - 1 and k < len(special):
            out.append(special[k])
            k += 1
    return out + special[k:]


def packed(special):
    """the special lines back to back, in three blocks with filler between them and behind the last"""
    fill = filler()
    third = (len(special) + 2) // 3
    out = list(fill[:3000])
    for b in range(3):
        out += special[b * third:(b + 1) * third] + fill[3000 + 2000 * b:5000 + 2000 * b]
    return out


def run(oracle, lines, knobs, framing="none", frames=None):
    """decode `frames` (default: the lines themselves) under force_sparse and compare with the oracle's Records of `lines`"""
    frames = lines if frames is None else frames
    data, offsets = synth.pack(frames)
    bdata, boffs = (data, offsets) if frames is lines else synth.pack(lines)
    dec = RFC5424Decoder()
    dec.set_launch_opts(force_sparse=True, **knobs)
    tables, keep = hl.decode_frames(dec, data, offsets, framing)
    hl.check(tables, dec, data, offsets, oracle.decode_batch(RFC5424, bdata, boffs), frames)
    return tables


@pytest.mark.parametrize("knobs", KNOBS, ids=KNOB_IDS)
def test_bench_shaped_corpus(oracle, knobs):
    """(a) 20 K lines of the bench corpus, its invalid lines included"""
    run(oracle, synth.rfc5424_lines(20000, cfg=2), knobs)


CASES = {"head-boundary": head_boundary_lines, "line-lengths": length_lines, "trim-points": trim_lines, "sd-and-garbage": sd_and_garbage_lines}


@pytest.mark.parametrize("knobs", KNOBS, ids=KNOB_IDS)
@pytest.mark.parametrize("place", [spread, packed], ids=["spread", "packed"])
@pytest.mark.parametrize("case", list(CASES))
def test_hand_made_lines(oracle, case, place, knobs):
    """(b) (c) (e) (f): few to the group and many to the group -- both sides of the dense fallback"""
    run(oracle, place(CASES[case]()), knobs)


@pytest.mark.parametrize("knobs", KNOBS, ids=KNOB_IDS)
def test_dense_fallback_and_back_in_long_chunks(oracle, knobs):
    """(f) chunks of 64 lines in groups of at most 16, four groups and more to the chunk: a wave meets the packed structured-data
    lines, stages the groups behind them dense and comes back to sparse inside one chunk.  (The plan keeps a named chunk size only
    when the batch holds two such chunks per wave: 36 K lines at one wave per CU.)"""
    lines = packed(sd_and_garbage_lines() + trim_lines()) + filler() * 3
    assert len(lines) >= 2 * 64 * hl.compute_units(RFC5424Decoder())
    run(oracle, lines, dict(knobs, chunk_lines=64, lines_per_group=16))


def test_every_alignment_of_the_first_line(oracle):
    """(d) a first line of 0 .. 31 bytes in front of a fixed set: every alignment of a line's start, and of the group's last two
    bytes, against the 16-byte chunks"""
    fixed = filler()[:150] + head_boundary_lines()[:8] + [line(tail=b"- " + BODY + b" "), line(tail=b"- m")]
    for k in range(32):
        run(oracle, [b"x" * k] + fixed, {"waves_per_cu": 1, "tile_cap": 2048})


@pytest.mark.parametrize("knobs", KNOBS, ids=KNOB_IDS)
@pytest.mark.parametrize("framing", ["line", "nul"])
def test_framings(oracle, framing, knobs):
    """(g) "\\n", "\\r\\n", a lone "\\r" in front of the "\\n", and NUL: the decoded line ends up to two bytes in front of the frame's end"""
    body = spread(trim_lines() + head_boundary_lines())
    if framing == "line":
        frames = [ln + (b"\r\n" if i % 3 == 0 else b"\r\r\n" if i % 7 == 0 else b"\n") for i, ln in enumerate(body)]
        frames[5], frames[6] = b"\n", b"\r\n"
    else:
        frames = [ln + b"\0" for ln in body]
        frames[5] = b"\0"
    run(oracle, [hl.stripped(f, framing) for f in frames], knobs, framing, frames)


@pytest.mark.parametrize("knobs", KNOBS, ids=KNOB_IDS)
def test_one_line_longer_than_the_tile(oracle, knobs):
    """(h) a 40 KiB line among short ones: a group of its own, parsed from global memory as in the whole-line kernel"""
    lines = list(filler())
    lines[77] = hl.BIG
    lines[4000] = hl.BIG + b" "
    run(oracle, lines, knobs)


def test_sparse_and_dense_tables_are_identical(oracle):
    """(i) the same batch under force_sparse and under no_sparse: every fixed column equal (ent_first is placed by wave-level allocation)"""
    import torch

    lines = spread(sd_and_garbage_lines() + trim_lines() + head_boundary_lines() + length_lines())
    data, offsets = synth.pack(lines)
    got = {}
    for name, opts in (("sparse", {"force_sparse": True}), ("dense", {"no_sparse": True})):
        dec = RFC5424Decoder()
        dec.set_launch_opts(**opts)
        tables, keep = hl.decode_frames(dec, data, offsets, "none")
        torch.cuda.synchronize(torch.device("cuda", dec.device))
        got[name] = {c: tables.column(c).cpu().numpy().copy() for c in ("meta", "ts", "hostname", "appname", "procid", "msgid", "msg", "full_msg", "ent_count")}
        want = oracle.decode_batch(RFC5424, data, offsets)
        hl.check(tables, dec, data, offsets, want, lines)
    for c in got["sparse"]:
        assert np.array_equal(got["sparse"][c], got["dense"][c]), c
