"""CPU: the escape carries of the two decode kernels (tests/escape_hazards.py).

  a) find_escaped16 (fg_sd2.hpp) on all 65536 backslash masks x both carries against a byte-wise model, and classify_tile itself on
     every one of them between a chunk that hands the carry in and a chunk of quotes that shows the carry handed out;
  b) find_escaped (fg_gelf2.hpp) on every run at every start bit, 200 000 random masks and pairs of words chained through the carry;
  c) every position class of escape_hazards through the wave emulation of the GELF fast form (WaveHost.gelf) and of the
     structured-data walk (fgs2_walk) at the geometries of test_wave_gelf_cpu / test_sd2_cpu: what is handled equals the oracle / the
     reference's state machine, and the hazard lines the fast forms can carry ARE handled.

The same streams run on the GPU in tests/test_gpu_escape_hazards.py."""
from __future__ import annotations

import ctypes as C
from collections import Counter

import numpy as np
import pytest

import escape_hazards as E
from flowgger_amd import synth
from test_sd2_cpu import check as sd_check, lib as sd_lib, walk as sd_walk  # noqa: F401  (sd_lib: the fixture)
from test_wave_gelf_cpu import check as gelf_check

GELF_FMT = 2
GELF_GEOMS = [dict(lines_per_group=32, tile_cap=12288), dict(lines_per_group=64, tile_cap=22528), dict(lines_per_group=16, tile_cap=6144),
              dict(lines_per_group=7, tile_cap=4096), dict(lines_per_group=48, tile_cap=16384)]
SD_GEOMS = [dict(), dict(lines_per_group=33, tile_cap=16384), dict(lines_per_group=7, tile_cap=6144), dict(lines_per_group=64, tile_cap=36864),
            dict(head_cap=1024, tile_cap=18432)]
LEDGER: Counter = Counter()  # (format, class, route) -> [lines, hazard lines, handled lines, handled hazard lines] as four keys


@pytest.fixture(scope="module")
def wave():
    import wave_binding

    return wave_binding.WaveHost()


def ptr(a):
    return C.c_void_p(a.ctypes.data)


def model(bs: np.ndarray, cin: np.ndarray, width: int):
    """escape_hazards.escaped_model, vectorised over the cases: -> (escaped mask, carry out)"""
    bs = bs.astype(np.uint64)
    esc = cin.astype(np.uint64) & np.uint64(1)
    out = np.zeros_like(bs)
    one = np.uint64(1)
    for i in range(width):
        out |= esc << np.uint64(i)
        esc = (one - esc) & ((bs >> np.uint64(i)) & one)
    return out, esc


def test_the_vectorised_model_is_the_byte_wise_one():
    rng = np.random.default_rng(3)
    bs = rng.integers(0, 1 << 63, 300, dtype=np.uint64) & rng.integers(0, 1 << 63, 300, dtype=np.uint64)
    cin = rng.integers(0, 2, 300).astype(np.uint64)
    got, carry = model(bs, cin, 64)
    for b, c, g, k in zip(bs, cin, got, carry):
        assert E.escaped_model(int(b), int(c), 64) == (int(g), int(k))
    assert E.escaped_model(0b0111, 0, 8) == (0b1010, 0) and E.escaped_model(0b0111, 1, 8) == (0b0101, 0)
    assert E.escaped_model(0b10000000, 0, 8) == (0, 1) and E.escaped_model(0b11000000, 0, 8) == (0b10000000, 0)


# ---- a) ---------------------------------------------------------------------------------------------------------------------------
def test_find_escaped16_on_every_mask(sd_lib):
    bs = np.tile(np.arange(65536, dtype=np.uint32), 2)
    cin = np.repeat(np.arange(2, dtype=np.uint32), 65536)
    out = np.zeros_like(bs)
    sd_lib.fgs2_find_escaped16(ptr(bs), ptr(cin), ptr(out), C.c_uint64(bs.size))
    want, _ = model(bs, cin, 16)
    bad = np.flatnonzero(out != want.astype(np.uint32))
    assert bad.size == 0, [(hex(int(bs[i])), int(cin[i]), hex(int(out[i])), hex(int(want[i]))) for i in bad[:5]]


def test_classify_tile_hands_every_carry_on(sd_lib):
    """three chunks per case: fifteen letters and a backslash (carry in) or a letter (none); the mask as backslashes, quotes everywhere
    else; sixteen quotes.  The real quotes of the second chunk are those no backslash escapes, and the first quote of the third is real
    exactly when the second ends in an even run -- the carry `classify_tile` computes with clz, between lanes (shfl_up1) and, every 64
    chunks, between trips (bcast)."""
    per = 1024  # cases per tile: 48 KiB, 48 trips
    masks = np.arange(65536, dtype=np.uint32)
    for cin in (0, 1):
        for m0 in range(0, 65536, per):
            m = masks[m0:m0 + per]
            tile = np.full((per, 48), ord("x"), np.uint8)
            if cin:
                tile[:, 15] = ord("\\")
            bits = ((m[:, None] >> np.arange(16, dtype=np.uint32)[None, :]) & 1).astype(bool)
            tile[:, 16:32] = np.where(bits, ord("\\"), ord('"'))
            tile[:, 32:48] = ord('"')
            # the cases shifted by 0, 1 or 2 chunks from tile to tile, so that the trip edge falls between other chunks of a case
            lead = 16 * ((m0 // per) % 3)
            flat = np.concatenate([np.full(lead, ord("x"), np.uint8), tile.reshape(-1)])
            flat = flat[:flat.size // 16 * 16]
            q16, b16 = np.zeros(flat.size // 16, np.uint16), np.zeros(flat.size // 16, np.uint16)
            rc = sd_lib.fgs2_classify(ptr(flat), C.c_uint32(flat.size), ptr(q16), ptr(b16))
            assert rc == (1 if m0 + per == 65536 else 0), sd_lib.fgs2_last_error()  # (0xFFFF: sixteen backslashes, the tile bails)
            q = q16[lead // 16:].reshape(per, 3)
            b = b16[lead // 16:].reshape(per, 3)
            esc, carry = model(m, np.full(per, cin, np.uint32), 16)
            keep = m != 0xFFFF  # (its carry is not computed: the tile takes the byte-wise walker)
            assert np.array_equal(b[:, 1], m.astype(np.uint16)) and np.array_equal(b[:, 0] != 0, np.full(per, bool(cin)))
            want1 = (~m & ~esc.astype(np.uint32) & 0xFFFF).astype(np.uint16)
            assert np.array_equal(q[keep, 1], want1[keep]), (cin, m0)
            want2 = (0xFFFF & ~carry.astype(np.uint32)).astype(np.uint16)
            bad = np.flatnonzero((q[:, 2] != want2) & keep)
            assert bad.size == 0, (cin, hex(int(m[bad[0]])), hex(int(q[bad[0], 2])), hex(int(want2[bad[0]])))


# ---- b) ---------------------------------------------------------------------------------------------------------------------------
def run_masks():
    out = []
    for n in range(65):
        for s in range(64):
            out.append((((1 << n) - 1) << s) & ((1 << 64) - 1))
    return np.array(out, np.uint64)


def test_find_escaped_on_runs_and_random_masks(wave):
    rng = np.random.default_rng(64)
    r = lambda: rng.integers(0, 1 << 64, 50_000, dtype=np.uint64)  # noqa: E731
    rnd = np.concatenate([r(), r() & r(), r() & r() & r(), r() | r()])
    assert rnd.size == 200_000
    runs = run_masks()
    # two runs in one word as well: the second one's parity must not depend on the first
    two = (runs[::7][:, None] | runs[None, 3::41]).reshape(-1)
    bs = np.concatenate([runs, runs, rnd, two])
    cin = np.concatenate([np.zeros(runs.size, np.uint64), np.ones(runs.size, np.uint64), rng.integers(0, 2, rnd.size + two.size).astype(np.uint64)])
    out = np.zeros_like(bs)
    wave.lib.fgw_find_escaped(ptr(bs), ptr(cin), ptr(out), C.c_uint64(bs.size))
    want, _ = model(bs, cin, 64)
    bad = np.flatnonzero(out != want)
    assert bad.size == 0, [(hex(int(bs[i])), int(cin[i]), hex(int(out[i])), hex(int(want[i]))) for i in bad[:5]]


def test_find_escaped_chained_through_the_carry(wave):
    """pairs (and one longer chain) of adjacent words, the carry taken from the top run of the word before as the word pass takes it;
    against the model run over all the bits at once.  A word of 64 backslashes is left out: its carry is not computed (the tile bails)."""
    rng = np.random.default_rng(65)
    full = (1 << 64) - 1
    pairs = []
    for n in range(1, 130):          # a run of n backslashes that ends at every bit of the second word / starts at every bit of the first
        for s in range(0, 64):
            v = ((1 << n) - 1) << s
            pairs.append((v & full, (v >> 64) & full))
    for _ in range(20_000):
        a = int(rng.integers(0, 1 << 64, dtype=np.uint64)) | (full << int(rng.integers(40, 64))) & full  # (a run at the top)
        pairs.append((a, int(rng.integers(0, 1 << 64, dtype=np.uint64)) | ((1 << int(rng.integers(0, 24))) - 1)))
    n_checked = 0
    for cin in (0, 1):
        for lo, hi in pairs:
            if lo == full or hi == full:
                continue
            bs = np.array([lo, hi], np.uint64)
            out = np.zeros(2, np.uint64)
            wave.lib.fgw_find_escaped_chain(ptr(bs), C.c_uint64(cin), ptr(out), C.c_uint64(2))
            want, _ = E.escaped_model(lo | (hi << 64), cin, 128)
            assert (int(out[0]), int(out[1])) == (want & full, want >> 64), (hex(lo), hex(hi), cin)
            n_checked += 1
    assert n_checked > 50_000
    words = rng.integers(0, 1 << 64, 4096, dtype=np.uint64) | (rng.integers(0, 1 << 64, 4096, dtype=np.uint64) << np.uint64(32))
    out = np.zeros_like(words)
    wave.lib.fgw_find_escaped_chain(ptr(words), C.c_uint64(0), ptr(out), C.c_uint64(words.size))
    big = 0
    for i, w in enumerate(words):
        big |= int(w) << (64 * i)
    want, _ = E.escaped_model(big, 0, 64 * words.size)
    assert all(int(out[i]) == (want >> (64 * i)) & full for i in range(words.size))


# ---- the plan ---------------------------------------------------------------------------------------------------------------------
def test_plan_covers_every_class_for_every_format_it_applies_to():
    for framing in (E.NONE, E.LINE, E.NUL):
        counts = E.plan(framing)
        print({f"{k[0]} {k[1]}{' (bail)' if len(k) == 3 else ''}": v for k, v in sorted(counts.items())})
        for cls, fmts in E.CLASSES.items():
            for fmt in (E.GELF, E.SD):
                assert (counts[(fmt, cls)] > 0) == (fmt in fmts), (framing, fmt, cls, counts[(fmt, cls)])
        for fmt in (E.GELF, E.SD):
            assert counts[(fmt, "fine", "bail")] == len(E.long_runs(fmt)) * E.WORD[fmt]
            by = {s.name: s for s in E.streams(fmt, framing)}
            # every run at every residue of the word; every run around every edge, -3 .. +3
            assert E.coverage(by[f"{fmt}-fine"]) == {(r, k) for r in E.short_runs(fmt) for k in range(E.WORD[fmt])}
            assert E.coverage(by[f"{fmt}-fine-bail"]) == {(r, k) for r in E.long_runs(fmt) for k in range(E.WORD[fmt])}
            edges = range(64, 768, 64) if fmt == E.GELF else (1024,)
            runs = (1, 2, 3, 4, 15, 16, 17, 31, 32, 33) if fmt == E.GELF else (1, 2, 3, 4, 5, 6, 7, 8, 15)
            assert E.coverage(by[f"{fmt}-coarse"]) >= {(r, e + d) for r in runs for e in edges for d in range(-3, 4) if e + d >= 18 + r}
            assert {k for _, k in E.coverage(by[f"{fmt}-round-up"])} == set(range(16))
            assert {k for _, k in E.coverage(by[f"{fmt}-toggle"])} == {0, 1, 63}
        head = {s.name: s for s in E.streams(E.SD, framing)}["sd-head-cap"]
        assert {k for _, k in E.coverage(head)} == set(range(1020, 1029))
        # ... with every alignment slack, and structured data that ends inside the head row in some lines, behind the cut in others
        assert {(a & 15, h.want) for a, h in zip(head.offsets, head.hz) if h.run} == {(k, w) for k in (0, 1, 15) for w in range(1020, 1029)}
        inside = [h.msg_at < E.HEAD_CAP - (a & 15) for a, h in zip(head.offsets, head.hz) if h.run and h.msg_at >= 0]
        assert any(inside) and not all(inside)
        member = {s.name: s for s in E.streams(E.GELF, framing)}["gelf-member"]
        assert {h.want for h in member.hz} == set(range(58, 71)) | set(range(122, 135))
        assert {h.tail for h in member.hz} == {e.decode() for e in E.ESCAPES} | {"none", "two"}
        # every line of the long-run streams that is not a hazard is an everyday line, and there are some
        for fmt in (E.GELF, E.SD):
            s = {s.name: s for s in E.streams(fmt, framing)}[f"{fmt}-fine-bail"]
            assert sum(1 for h in s.hz if not h.run) >= len(s.hz) // 6
    # the 768-byte lines of GELF's coarse stream: the geometries of the emulation give a lane 1, 2, 3, 4 and 6 words of the word pass
    wn = {-(-min(g["lines_per_group"], g["tile_cap"] // 768) * 12 // 64) for g in GELF_GEOMS}
    assert wn == {1, 2, 3, 4, 6}


def test_fine_stream_meets_every_residue_of_a_fused_tile():
    """the tiles of the fused kernels start anywhere (escape_hazards.fused_residue): at the geometries fg::fused_geometry plans for GELF's
    everyday line length -- the constant 3 KiB kernel, the run-time one, the link-bound one of fg_frame_decode_batch -- every run of the
    `fine` stream still meets every residue 0 .. 63 of the tile's words"""
    from fuse_binding import FuseHost

    host = FuseHost()
    want = {(r, k) for r in E.short_runs(E.GELF) for k in range(64)}
    for framing in (E.LINE, E.NUL):
        s = {s.name: s for s in E.streams(E.GELF, framing)}["gelf-fine"]
        for pin in (dict(), dict(flags=1), dict(link_bound=True)):  # (1 = FG_LO_GELF_GENERIC)
            g = host.geometry(GELF_FMT, 300, **pin)
            assert g["ok"] and g["S"] >= 1536
            got = {(h.run, E.fused_residue(s, i, g["S"])) for i, h in enumerate(s.hz) if h.run}
            assert got >= want, (framing, pin, g["S"], sorted(want - got)[:8])


# ---- c) ---------------------------------------------------------------------------------------------------------------------------
def tally(fmt, cls, route, hz, handled):
    run = np.array([h.run != 0 for h in hz])
    LEDGER[(fmt, cls, route, "lines")] += len(hz)
    LEDGER[(fmt, cls, route, "hazards")] += int(run.sum())
    LEDGER[(fmt, cls, route, "handled")] += int(np.asarray(handled, bool).sum())
    LEDGER[(fmt, cls, route, "hazards handled")] += int((np.asarray(handled, bool) & run).sum())


def gelf_framed(wave, oracle, s: E.Stream, **geom):
    """test_wave_gelf_cpu.check for the frames of a raw stream: every handled row equals the oracle's decode of the bare line"""
    offsets = np.array(s.offsets, np.uint64)
    pad = np.concatenate([np.frombuffer(s.raw, np.uint8), np.zeros(64, np.uint8)])
    tab, handled = wave.gelf(pad, offsets, strip=s.framing, **geom)
    bdata, boffs = synth.pack(s.lines())
    oblob, ooffs = oracle.decode_batch(GELF_FMT, bdata, boffs)
    blob, offs = tab.serialize(GELF_FMT, pad, offsets)
    for i in np.nonzero(handled)[0]:
        got = blob[int(offs[i]):int(offs[i + 1])].tobytes()
        want = oblob[int(ooffs[i]):int(ooffs[i + 1])].tobytes()
        assert got == want, f"{s.name} frame {i}: {s.hz[i].line[:200]!r}\n  wave   {got[:300]!r}\n  oracle {want[:300]!r}"
    return handled


@pytest.mark.parametrize("framing", [E.NONE, E.LINE, E.NUL], ids=["bare", "line", "nul"])
def test_gelf_classes_on_the_emulation(wave, oracle, framing):
    """every class through decode_tile: handled rows equal the oracle's Records; outside the long-run streams every hazard line with an
    even run of at most 62 backslashes is handled by the fast form itself"""
    for s in E.streams(E.GELF, framing):
        for geom in (GELF_GEOMS if framing == E.NONE else GELF_GEOMS[2:4]):
            if framing == E.NONE:
                handled = gelf_check(wave, oracle, s.lines(), **geom)
            else:
                handled = gelf_framed(wave, oracle, s, **geom)
            tally(E.GELF, s.cls + (" (bail)" if s.bail else ""), f"emulation {('bare', 'line', 'nul')[framing]}", s.hz, handled)
            if s.bail:
                continue
            for i, h in enumerate(s.hz):
                if h.must(E.GELF):
                    assert handled[i], f"{s.name} {geom}: the fast form handed back run {h.run} at {h.q} tail {h.tail}: {h.line[:120]!r}"
    rows = {k[:3] for k in LEDGER if k[0] == E.GELF}
    for k in sorted(rows):
        print(k, {n: LEDGER[k + (n,)] for n in ("lines", "hazards", "handled", "hazards handled")})


def test_sd_classes_on_the_emulation(sd_lib):
    """every class through classify_tile + group_walk: what is handled equals the reference's state machine; outside the long-run
    streams every hazard line with an even run of at most 15 backslashes is handled.  With HEAD staging that holds for the lines whose
    structured data ends inside the head row: a line whose terminal `] ` lies behind the cut is handed back for the second look
    (fg_sd2.hpp:263 `if (!line_end_known) return ev;` and :528, "the head ends here: give the line back").  (The emulation's driver
    knows no terminators: the framed streams of the structured-data walk run on the device only.)"""
    for s in E.streams(E.SD, E.NONE):
        for geom in SD_GEOMS:
            got, ref = sd_walk(sd_lib, s.lines(), **geom)
            sd_check(sd_lib, s.lines(), **geom)
            handled = got["handled"].astype(bool)
            route = "emulation head rows" if geom.get("head_cap") else "emulation whole lines"
            tally(E.SD, s.cls + (" (bail)" if s.bail else ""), route, s.hz, handled)
            if s.bail:
                # a chunk of sixteen backslashes takes the whole tile to the byte-wise walker
                assert got["bailed"].any() and not handled[got["bailed"].astype(bool)].any()
                continue
            for i, h in enumerate(s.hz):
                if not h.must(E.SD):
                    continue
                if geom.get("head_cap") and h.msg_at >= geom["head_cap"] - (s.offsets[i] & 15):
                    continue
                assert handled[i], f"{s.name} {geom}: the fast form handed back run {h.run} at {h.q} tail {h.tail}: {h.line[:120]!r}"
    rows = {k[:3] for k in LEDGER if k[0] == E.SD}
    for k in sorted(rows):
        print(k, {n: LEDGER[k + (n,)] for n in ("lines", "hazards", "handled", "hazards handled")})
