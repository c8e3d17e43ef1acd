"""GPU tests of the regrouped RFC3164 decode (flowgger_amd/csrc/fg_rfc3164.hip: k_rfc3164 hands the lines of a slow shape to per-class
lists, k_rfc3164_perm stages 64 listed lines as rows of one LDS tile) and of the pinned raw streams the fused frame + decode launch
declines.  Every comparison is byte for byte on the canonical Record blob against the oracle; the corpora are built from the kernels'
own arithmetic, restated here (tile_cap_of, list_cap_of, rows_of) and asserted, so that a test cannot pass because its lines never
reached the path it is about."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from flowgger_amd import LTSVDecoder, RFC3164Decoder, RFC5424Decoder, synth, tzdb
from flowgger_amd import _lib as L
from flowgger_amd.record import DecodeError, parse_canonical
from flowgger_amd.tables import DeviceTables, HostTables
from gpu_util import assert_same, device_path
from oracle_binding import Oracle
from test_gpu_parity import RFC3164_CONFIG, RFC3164_YEAR
from test_gpu_round6 import check_rows, expected_frames, stream_of
from test_rfc3164_cpu import fuzz_lines

pytestmark = pytest.mark.gpu

WAVE = 64
SUB_LISTS = 64          # fg_rfc3164.hip kSubLists: a source wave appends to list (its index & 63) of the line's class
MONTHS = ["Jan", "Feb", "Mar", "Apr", "May", "Jun", "Jul", "Aug", "Sep", "Oct", "Nov", "Dec"]
COLUMNS = ("meta", "ts", "hostname", "msg")
PAD = b"lorem ipsum dolor sit amet consectetur adipiscing elit sed do eiusmod tempor incididunt ut labore et dolore magna aliqua "


@pytest.fixture(scope="module")
def oracle():
    o = Oracle()
    o.set_rfc3164(RFC3164_YEAR, tzdb.default_table())
    return o


@pytest.fixture(scope="module")
def dec():
    d = RFC3164Decoder(RFC3164_CONFIG)
    yield d
    d.set_launch_opts()


# ---------------------------------------------------------------------------------------------
# the kernels' arithmetic, restated
# ---------------------------------------------------------------------------------------------
def tile_cap_of(nbytes, n, override):
    """fg_tile_cap.hpp pick_tile_cap for the RFC3164 decoder (at most 56 KiB, a margin of 2/16)"""
    if 1024 <= override <= 56 * 1024:
        return (override + 1023) // 1024 * 1024
    avg = (nbytes + n - 1) // n
    want = (64 * avg * 18 // 16 + 512 + 1023) // 1024 * 1024
    return min(max(want, 4096), 56 * 1024)


def list_cap_of(n):
    """fg_rfc3164.hip r3164_list_cap: records a list holds"""
    c = (n // 2 + SUB_LISTS - 1) // SUB_LISTS
    return max((c + WAVE - 1) // WAVE * WAVE, WAVE)


def rows_of(offsets, idx):
    """the LDS row of every listed line: from the line's 16-byte boundary, rounded up to 16, 16 for an empty line"""
    o = offsets.astype(np.int64)
    want = (o[idx + 1] - o[idx]) + (o[idx] & 15)
    return np.maximum((want + 15) & ~15, 16)


def wave_span(offsets, w):
    o = offsets.astype(np.int64)
    g0, g1 = w * WAVE, min((w + 1) * WAVE, len(o) - 1)
    return int((o[g1] - (o[g0] & ~15) + 15) & ~15)


def padded(head: str, length: int) -> bytes:
    b = head.encode()
    assert len(b) <= length, (head, length)
    return (b + PAD * (length // len(PAD) + 1))[:length]


def std_line(i: int, length: int) -> bytes:
    """the everyday shape (key 0: parsed where it lies), at least 19 bytes"""
    if length < 40:
        return padded(f"{MONTHS[i % 12]} {1 + i % 28:2d} {i % 24:02d}:{i * 7 % 60:02d}:{i * 11 % 60:02d} h m", length)
    return padded(f"<{i % 192}>{MONTHS[i % 12]} {1 + i % 28:2d} {i % 24:02d}:{i * 7 % 60:02d}:{i * 11 % 60:02d} h{i % 997} app[{i}]: ", length)


def slow_line(cls: int, k: int, length: int) -> bytes:
    """a line of a slow shape whose FIRST SIXTEEN BYTES are its own: the priority (one, two and three digits), the date and the time
    (class 0: zone-tagged, keys 2 / 3) or the priority, the hostname and the year (class 1: the custom form, key 4) change with k"""
    pri = (k * 37 + 3) % 192
    mon, day, hh, mm, ss = MONTHS[(k * 5) % 12], 1 + (k * 3) % 28, (k * 7) % 24, (k * 13) % 60, (k * 11) % 60
    if cls == 0:
        return padded(f"<{pri}>{mon} {day:2d} {hh:02d}:{mm:02d}:{ss:02d} Europe/Paris host{k} app[{1000 + k}]: ", length)
    return padded(f"<{pri}>h{k}: {1990 + k % 40} {mon} {day} {hh:02d}:{mm:02d}:{ss:02d}: app{k}: ", length)


def build_batch(n_src, per_wave, make_slow, short_len, filler_len):
    """waves 0, 64, 128 ... (n_src of them: ONE list per class) hold per_wave[s] slow lines each at scattered lanes among short everyday
    lines; every other wave holds everyday lines of filler_len bytes.  Returns (lines, indices of the slow lines)."""
    n_waves = SUB_LISTS * (n_src - 1) + 1
    lines, slow, k = [], [], 0
    for w in range(n_waves):
        src = w % SUB_LISTS == 0
        lanes = {(j * 5 + 2) % WAVE for j in range(per_wave[w // SUB_LISTS])} if src else set()
        for lane in range(WAVE):
            i = w * WAVE + lane
            if lane in lanes:
                slow.append(i)
                lines.append(make_slow(k))
                k += 1
            elif src:
                lines.append(std_line(i, short_len(i)))
            else:
                lines.append(std_line(i, filler_len(i)))
    return lines, np.array(slow, np.int64)


def run_modes(dec, oracle, lines, tile_cap, modes=(1, 2)):
    """the batch through the regrouped (1) and the plain (2) kernel: each against the oracle, the columns of the two bit for bit"""
    data, offsets = synth.pack(lines)
    oblob, ooffs = oracle.decode_batch(dec.fmt, data, offsets, None)
    cols = {}
    for mode in modes:
        dec.set_launch_opts(rfc3164_regroup=mode, tile_cap=tile_cap)
        tables, _, _ = device_path(dec, data, offsets)
        host = tables.to_host()
        blob, offs = host.serialize(dec.fmt, data, offsets, cfg=dec._cfg)
        assert_same(blob, offs, oblob, ooffs, [ln[:100] for ln in lines])
        n = len(lines)
        cols[mode] = [host.a[c][: n * (2 if c in ("hostname", "msg") else 1)].copy() for c in COLUMNS]
    dec.set_launch_opts()
    for mode in modes[1:]:
        for name, a, b in zip(COLUMNS, cols[modes[0]], cols[mode]):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"column {name}: regroup {modes[0]} != {mode}"
    return data, offsets, oblob, ooffs


def assert_listed(lines, offsets, slow, n_src, per_wave, tile_cap):
    """what makes the slow lines reach k_rfc3164_perm, all in the first workgroup(s) of one list: their source waves are staged
    (span <= tile), regroup (fewer than 32 slow lanes) and the list has room"""
    n = len(lines)
    cap = tile_cap_of(int(offsets[-1]), n, tile_cap)
    for s in range(n_src):
        assert per_wave[s] < 32
        assert wave_span(offsets, s * SUB_LISTS) <= cap, (s, wave_span(offsets, s * SUB_LISTS), cap)
    assert len(slow) <= list_cap_of(n)
    return cap


# ---------------------------------------------------------------------------------------------
# A. listed rows that outgrow the tile and 64 KiB
# ---------------------------------------------------------------------------------------------
SLOW_LEN = 2033    # a row of 2048 bytes at every alignment: the prefix sum of the rows is 2048 k, (2048 k) & 0xFFFF the start of row k mod 32
MID_LEN = 1025     # a row of 1040 bytes at every alignment


def outgrow_case(cls, tile_cap, records, mixed):
    """40 records = two source waves of 20 slow lines, 64 = four of 16.  The source waves must fit the tile to be staged at all: at
    20 KiB a wave holds 8 slow lines among 19-byte ones (five / eight waves), and under the library's own choice the other waves hold
    800-byte everyday lines so that the batch average asks for the 56 KiB tile."""
    if tile_cap == 20480:
        per_wave, short_len = [8] * (records // 8), (lambda i: 19 + i % 3)
    else:
        per_wave, short_len = ([20, 20] if records == 40 else [16] * 4), (lambda i: 60 + i * 13 % 21)
    filler_len = (lambda i: 800 + i % 7) if tile_cap == 0 else (lambda i: 40 + i * 13 % 31)
    length = (lambda k: MID_LEN if k % 3 == 0 else SLOW_LEN) if mixed else (lambda k: SLOW_LEN)
    lines, slow = build_batch(len(per_wave), per_wave, lambda k: slow_line(cls, k, length(k)), short_len, filler_len)
    return lines, slow, per_wave


OUTGROW = [(cls, cap, rec, False) for cls in (0, 1) for cap in (0, 57344, 20480) for rec in (40, 64)] + [(0, 57344, 64, True), (1, 0, 64, True)]


@pytest.mark.parametrize("cls,tile_cap,records,mixed", OUTGROW,
                         ids=[f"{'zone' if c == 0 else 'custom'}-cap{t}-{r}rec{'-mixed' if m else ''}" for c, t, r, m in OUTGROW])
def test_listed_rows_past_the_tile_and_64k(oracle, dec, cls, tile_cap, records, mixed):
    """One perm workgroup gets 40 / 64 rows of 2048 bytes: 80 / 128 KiB against a tile of at most 56 KiB.  The rows that do not fit
    (and the lanes without a record, whose prefix sum is the total) have a row offset of 64 KiB and more; whatever the kernel
    publishes for them must not reach the staging stores -- an offset taken modulo 64 KiB is the START of a staged row (row k mod 32;
    mid-row in the mixed case), and the head of another line copied there changes that line's priority, timestamp or verdict: every slow
    line's first sixteen bytes are its own.  At 20 KiB the targets past row 9 are not in the tile at all and those rows are read from
    global memory."""
    lines, slow, per_wave = outgrow_case(cls, tile_cap, records, mixed)
    data, offsets = synth.pack(lines)
    cap = assert_listed(lines, offsets, slow, len(per_wave), per_wave, tile_cap)
    assert len(slow) == records
    rows = rows_of(offsets, slow)
    if mixed:
        assert set(rows.tolist()) == {2048, 1040} and int(rows.sum()) < (1 << 20)
    else:
        assert np.all(rows == 2048)
        assert cap // 2048 == {0: 28, 57344: 28, 20480: 10}[tile_cap]
    assert int(rows.sum()) > 65536 + 2048  # rows past 64 KiB, and the total (the lanes without a record) past it too
    heads = {lines[i][:16] for i in slow}
    assert len(heads) == records, "two slow lines share their first sixteen bytes"
    data, offsets, oblob, ooffs = run_modes(dec, oracle, lines, tile_cap)
    recs = [parse_canonical(oblob[int(ooffs[i]):int(ooffs[i + 1])].tobytes()) for i in slow]
    ok = [r for r in recs if not isinstance(r, DecodeError)]
    assert len(ok) >= 0.9 * records, f"only {len(ok)} of {records} slow lines decode"
    assert len({(r.facility, r.severity, r.ts) for r in ok}) >= 32


# ---------------------------------------------------------------------------------------------
# B. thresholds and geometry
# ---------------------------------------------------------------------------------------------
ROW_SIZES = [16, 240, 256, 272, 496, 512, 528, 1024]


def rows_batch(pattern, odd):
    """three source waves of 22 + 21 + 21 custom-form lines = ONE full perm workgroup whose rows are pattern[k % len].  odd = False:
    every line a multiple of 16 bytes (rows == lengths); True: lines of every length, each listed line cut to its row from where it
    happens to start."""
    per_wave = [22, 21, 21]
    n_waves = SUB_LISTS * 2 + 1
    lines, slow, k, off = [], [], 0, 0
    for w in range(n_waves):
        src = w % SUB_LISTS == 0
        lanes = {(j * 5 + 2) % WAVE for j in range(per_wave[w // SUB_LISTS])} if src else set()
        for lane in range(WAVE):
            i = w * WAVE + lane
            if lane in lanes:
                row = pattern[k % len(pattern)]
                length = max(row - (off & 15) - (k % 16 if odd else 0), 0)
                ln = b"" if length == 0 else slow_line(1, k, length) if length >= 48 else (b"x" * length)  # (no capital: key 4)
                slow.append(i)
                k += 1
            else:
                ln = std_line(i, (35 + i * 13 % 41) if odd else 32 + 16 * (i % 3))
            lines.append(ln)
            off += len(ln)
    return lines, np.array(slow, np.int64), per_wave


@pytest.mark.parametrize("odd", [False, True], ids=["aligned", "every-alignment"])
@pytest.mark.parametrize("long_rows", ["many", "few"])
def test_row_size_thresholds_of_the_perm_kernel(oracle, dec, odd, long_rows):
    """rows of exactly 16 (an empty line), 240, 256, 272, 496, 512, 528 and 1024 bytes in one full workgroup.  `many`: more than 24 rows
    above 256 bytes (their second 256 bytes ride in the first round trip for the first 24 only; the others and everything past 512
    bytes take the `rest` passes); `few`: at most 24."""
    pattern = ROW_SIZES if long_rows == "many" else [16, 240, 256, 240, 272, 256, 1024, 16, 496, 240, 256, 512, 528, 240, 256, 16]
    lines, slow, per_wave = rows_batch(pattern, odd)
    data, offsets = synth.pack(lines)
    assert_listed(lines, offsets, slow, 3, per_wave, 57344)
    rows = rows_of(offsets, slow)
    assert len(slow) == 64 and rows.tolist() == [pattern[k % len(pattern)] for k in range(64)]
    assert set(ROW_SIZES) <= set(rows.tolist())
    n_long = int((rows > 256).sum())
    assert (n_long > 24) if long_rows == "many" else (0 < n_long <= 24)
    assert int((rows > 512).sum()) > 0 and int(rows.sum()) <= 57344
    run_modes(dec, oracle, lines, 57344)


@pytest.mark.parametrize("tile_cap", [4096, 20480])
@pytest.mark.parametrize("over", [0, 16])
def test_rows_that_fill_the_tile_exactly(oracle, dec, tile_cap, over):
    """64 equal rows that sum to tile_cap exactly (all of them staged), and the same with ONE row sixteen bytes longer, the last
    listed line of the last source wave: that row -- and, should the waves have appended in another order, those behind it -- is
    read from global memory."""
    row = tile_cap // 64
    per_wave = [22, 21, 21]
    lines, slow = build_batch(3, per_wave, lambda k: slow_line(1, k, row + (over if k == 63 else 0)), lambda i: 32, lambda i: 48)
    data, offsets = synth.pack(lines)
    assert_listed(lines, offsets, slow, 3, per_wave, tile_cap)
    assert not np.any(offsets[slow].astype(np.int64) & 15)
    rows = rows_of(offsets, slow)
    assert int(rows.sum()) == tile_cap + over and int(rows[:63].sum()) + row == tile_cap
    run_modes(dec, oracle, lines, tile_cap)


@pytest.fixture(scope="module")
def sweep_corpus(oracle):
    rng = np.random.default_rng(3164)
    base = synth.rfc3164_lines(5000) + fuzz_lines(2800, 31)
    base += [b"", b"<", b"<1", b"<12>", b"A", b"Aug", b"Aug 6 11:15:24 Host-With-Capital app: m", b"<34>2019 Aug 6 11:15:24 UTC h a: m", b"<5>1234x", b"a: b: ",
             b"Aug 6 11:15:24 " + b"h" * 9000 + b" long hostname token", b"<190>Oct  1 00:00:00 Europe/Paris h app[1]: " + b"x" * 70_000]
    longs = []
    for k in range(100):
        length = int(rng.integers(600, 3001))
        longs.append(slow_line(0, k, length) if k % 3 == 0 else slow_line(1, k, length) if k % 3 == 1 else std_line(k, length))
    lines = list(base)
    for k, ln in enumerate(longs):  # sprinkled: a wave holds one or two of them among everyday lines
        lines.insert(int(rng.integers(0, len(lines))), ln)
    data, offsets = synth.pack(lines)
    oblob, ooffs = oracle.decode_batch(L.FG_RFC3164, data, offsets, None)
    return lines, data, offsets, oblob, ooffs


def test_geometry_sweep_of_both_kernels(oracle, dec, sweep_corpus):
    """tile_cap 1 KiB (most waves read global memory) .. 56 KiB and the library's own, regrouped and plain: ten runs over the synthetic
    corpus, structured fuzz, the shape key's edge cases and a hundred lines of 600 .. 3000 bytes -- each equal to the oracle, all ten
    alike column by column"""
    lines, data, offsets, oblob, ooffs = sweep_corpus
    n = len(lines)
    assert 7900 <= n <= 8100
    first = None
    for tile_cap in (1024, 4096, 20480, 57344, 0):
        for mode in (1, 2):
            dec.set_launch_opts(rfc3164_regroup=mode, tile_cap=tile_cap)
            tables, _, _ = device_path(dec, data, offsets)
            host = tables.to_host()
            blob, offs = host.serialize(dec.fmt, data, offsets, cfg=dec._cfg)
            assert_same(blob, offs, oblob, ooffs, [ln[:100] for ln in lines])
            cols = [host.a[c][: n * (2 if c in ("hostname", "msg") else 1)].copy() for c in COLUMNS]
            if first is None:
                first = cols
            for name, a, b in zip(COLUMNS, first, cols):
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"column {name}: tile_cap {tile_cap} regroup {mode}"
    dec.set_launch_opts()


def test_regrouped_frames_with_terminators(oracle, dec):
    """frames (FG_FRAME_LINE: terminators stripped in the kernel) through the lists: a listed line that ends in \\r\\n, a listed line
    that is not valid UTF-8, regrouping forced on a small stream"""
    import torch

    lines = [std_line(i, 60 + i % 30) for i in range(64)] + synth.rfc3164_lines(3000)
    crlf, bad = 5, 9
    lines[crlf] = slow_line(0, 1, 300) + b"\r"
    lines[bad] = slow_line(1, 2, 200)[:150] + b"\xff\xfe not utf-8"
    lines[11], lines[12] = slow_line(0, 3, 700), slow_line(1, 4, 90)
    stream = b"".join(ln + b"\n" for ln in lines)
    raw = torch.frombuffer(bytearray(stream + b"\0" * 32), dtype=torch.uint8).cuda()[:len(stream)]
    d_off, d_bad, nf = dec.frame_device(raw, L.FG_FRAME_LINE)
    assert nf == len(lines)
    off = d_off[:nf + 1].cpu().numpy().astype(np.uint64)
    assert wave_span(off, 0) <= tile_cap_of(len(stream), nf, 0)  # the first wave is staged: its four slow lines are listed
    good = [ln[:-1] if ln.endswith(b"\r") else ln for ln in lines]
    gdata, goffs = synth.pack(good)
    oblob, ooffs = oracle.decode_batch(dec.fmt, gdata, goffs)
    data = np.frombuffer(stream + b"\0" * 32, np.uint8)
    cols = {}
    for mode in (1, 2):
        dec.set_launch_opts(rfc3164_regroup=mode)
        tables = DeviceTables(nf, 16, raw.device)
        dec.decode_frames_device(raw, d_off, nf, tables, L.FG_FRAME_LINE, d_bad)
        torch.cuda.synchronize()
        host = tables.to_host()
        blob, offs = host.serialize(dec.fmt, data, off, 0, nf)
        assert host.status[bad] == L.FG_ST_BAD_UTF8
        for i in range(nf):
            if i != bad:
                assert blob[int(offs[i]):int(offs[i + 1])].tobytes() == oblob[int(ooffs[i]):int(ooffs[i + 1])].tobytes(), (mode, i, lines[i][:80])
        cols[mode] = [host.a[c][: nf * (2 if c in ("hostname", "msg") else 1)].copy() for c in COLUMNS]
    dec.set_launch_opts()
    for name, a, b in zip(COLUMNS, cols[1], cols[2]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), name


# ---------------------------------------------------------------------------------------------
# C. pinned streams that the fused launch declines
# ---------------------------------------------------------------------------------------------
ROW_COLUMNS = ("meta", "ts", "hostname", "appname", "procid", "msgid", "msg", "full_msg", "ent_count")


def declined_case(name):
    if name == "rfc5424-long-tail":
        return RFC5424Decoder(), None, synth.rfc5424_lines(4_000, cfg=5, sd=True, long_tail=True), True
    if name == "ltsv-long-tail":
        return LTSVDecoder(synth.LTSV_CONFIG), synth.LTSV_CONFIG, synth.ltsv_lines(4_000, invalid_frac=0.005, long_tail=True), True
    return RFC3164Decoder(RFC3164_CONFIG), None, synth.rfc3164_lines(20_000), False


@pytest.mark.parametrize("name", ["rfc5424-long-tail", "ltsv-long-tail", "rfc3164"])
def test_pinned_streams_the_fused_launch_declines(oracle, name):
    """fg_frame_decode_batch on a PINNED chunk whose lines the one-launch form does not take -- RFC3164 (no fused kernel) and lines of
    768 bytes and more on average (the head-staging kernels) -- : fg_frame_decode_device answers FG_ERR_UNSUPPORTED and the chunk is
    uploaded, framed and decoded by the separate kernels.  Frames, `used`, every valid frame's Record against the oracle; the path
    taken is not the fused one whether or not it was allowed, and both give the same tables.
    (The launch is planned from the average line of the ctx's LAST chunk of a MiB or more -- 200 bytes before it has seen one --, so
    the run with the fused form switched off comes first: from then on the ctx knows the stream's line length.)"""
    dec, cfg, lines, long_tail = declined_case(name)
    fmt = dec.fmt
    lib = L.lib()
    raw = stream_of(lines, L.FG_FRAME_LINE, crlf_every=9, empty_every=1001, damage_every=89, tail=b"tail without a terminator")
    assert len(raw) >= 1 << 20
    p = C.c_void_p()
    L.check(lib.fg_alloc_pinned(len(raw) + 64, C.byref(p)), "fg_alloc_pinned")
    try:
        buf = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), (len(raw) + 64,))
        buf[:] = 0x0A
        buf[: len(raw)] = np.frombuffer(raw, np.uint8)
        for final in (True, False):
            starts, ends, valid = expected_frames(oracle, raw, L.FG_FRAME_LINE, final)
            if long_tail:
                assert int(ends[-1]) >= 768 * len(starts), "the corpus' average line is below the head-staging threshold"
            seen = {}
            for no_fused in (True, False):
                dec.set_launch_opts(no_fused_framing=no_fused)
                st = L.fg_tables()
                off = C.c_void_p()
                nf, used = C.c_uint64(), C.c_uint64()
                L.check(lib.fg_frame_decode_batch(dec._ctx, fmt, L.FG_FRAME_LINE, p, len(raw), int(final), C.byref(st), C.byref(off), C.byref(nf),
                                                  C.byref(used)), "fg_frame_decode_batch")
                path = int(lib.fg_last_host_path(dec._ctx))
                assert path != L.FG_PATH_FRAME_FUSED and path != 0, (final, no_fused, path)
                n = int(nf.value)
                assert n == len(starts), (final, no_fused)
                assert int(used.value) == (int(ends[-1]) if n else 0)
                offs = np.ctypeslib.as_array(C.cast(off, C.POINTER(C.c_uint64)), (n + 1,)).copy()
                tab = HostTables.from_struct(st)
                check_rows(oracle, fmt, cfg, dec._cfg, raw, L.FG_FRAME_LINE, starts, ends, valid, tab, offs)
                blob, boffs = tab.serialize(fmt, np.frombuffer(raw + b"\0" * 32, np.uint8), np.ascontiguousarray(offs, np.uint64), 0, n, cfg=dec._cfg)
                seen[no_fused] = (offs, blob, boffs, [tab.a[c][: n * (1 if c in ("meta", "ts", "ent_count") else 2)].copy() for c in ROW_COLUMNS])
            a, b = seen[True], seen[False]
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
            for cname, x, y in zip(ROW_COLUMNS, a[3], b[3]):
                assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"column {cname}: fused allowed != switched off"
    finally:
        dec.set_launch_opts()
        lib.fg_free_pinned(p)
