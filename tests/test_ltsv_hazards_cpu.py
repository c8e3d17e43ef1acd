"""CPU: the streams of tests/ltsv_hazards.py -- a byte at every boundary of the LTSV kernel -- before they reach the GPU
(tests/test_gpu_ltsv_hazards.py):

  a) every aimed position is where its line says (check_invariants, from the packed offsets), no class is empty, and the sweeps
     that are exhaustive by design are complete;
  b) the oracle gives every line exactly the Record or the error it was BUILT to give: no line is "whatever the oracle says",
     which is what keeps the byte comparison of the GPU test from being vacuous;
  c) the geometry the generator aims at is the one in the sources (the head size, the rows behind it, the TAB window, the records):
     the next change of one of them fails here instead of quietly disarming a sweep;
  d) the `records` class straddles the record-fit condition from both sides: with `<` for `<=` the lines aimed AT the limit, and
     only they, would change."""
from __future__ import annotations

import re
from pathlib import Path

import pytest

import ltsv_hazards as H
from flowgger_amd import synth
from flowgger_amd.record import DecodeError, parse_canonical

LTSV = 1
CSRC = Path(__file__).resolve().parent.parent / "flowgger_amd" / "csrc"
FRAMINGS = [H.NONE, H.LINE, H.NUL]
IDS = ["bare", "line", "nul"]


def aimed(s: H.Stream):
    """(absolute start, line) of the aimed lines"""
    return [(a, h) for a, h in zip(s.offsets, s.ln) if h.aim]


def by_name(framing: int):
    return {s.name: s for s in H.streams(framing)}


# ---- a) -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("framing", FRAMINGS, ids=IDS)
def test_invariants_and_ledger(framing):
    for s in H.streams(framing):
        H.check_invariants(s)
    led = H.ledger(framing)
    print({k: {"lines": v[0], "aimed": v[1]} for k, v in led.items()})
    assert set(led) == set(H.CLASSES)
    for cls, (n, k) in led.items():
        assert n > 0 and k > 0, cls


@pytest.mark.parametrize("framing", FRAMINGS, ids=IDS)
def test_exhaustive_sweeps_are_complete(framing):
    S = by_name(framing)
    t = len(H.term_of(framing))
    al16, q4 = set(range(16)), set(range(4))
    # tab-window: the first TAB at every index 0 .. 200 = every bit of the window, behind 0 .. 3 refills, for every start mod 16
    first = [(a, h) for a, h in aimed(S["tab-index"])]
    assert {(h.pos, a & 15) for a, h in first} == {(i, r) for i in range(201) for r in al16}
    assert {(h.pos % H.TAB_WINDOW, a & 15) for a, h in first} == {(b, r) for b in range(H.TAB_WINDOW) for r in al16}
    parts = aimed(S["tab-parts"])
    starts = {h.pos for _, h in parts if h.aim == "search-start"}
    assert starts == set(range(1, 132)) and {p % H.TAB_WINDOW for p in starts} == set(range(H.TAB_WINDOW))
    assert {H.TAB_WINDOW - 1, H.TAB_WINDOW, H.TAB_WINDOW + 1, 2 * H.TAB_WINDOW - 1, 2 * H.TAB_WINDOW, 2 * H.TAB_WINDOW + 1} <= starts
    runs = {(h.want[1], "front" if h.pos == 0 else "back" if h.pos + h.want[1] == len(h.line) else "middle", a & 15)
            for a, h in parts if h.aim == "empty-run"}
    assert runs == {(n + (w == "middle"), w, r) for n in H.EMPTY_RUNS for w in ("front", "middle", "back") for r in al16}
    for aim in ("tab-first", "tab-last"):
        assert {a & 15 for a, h in parts if h.aim == aim} == al16
    assert sum(1 for _, h in parts if h.aim == "no-tab") >= 16
    # colon
    col = aimed(S["colon"])
    assert {(h.aim, h.want[1]) for _, h in col if h.want[0] == "part" and h.aim != "value-colons"} == \
        {(w, c) for w in ("colon-first", "colon-middle", "colon-last") for c in H.COLON_AT}
    assert {15, 16, 17} <= set(H.COLON_AT)
    nxt = {(h.aim, h.want[1], (a + h.pos) & 3) for a, h in col if h.want[0] == "next"}
    assert {(w, n) for w, n, _ in nxt} == {(w, n) for w in ("bare-then-part", "bare-then-line") for n in H.BARE_LEN}
    # ... the neighbour's ':' inside the bare part's own 16-byte window wherever the part is short enough for that
    inside = {(h.aim, h.want[1]) for _, h in col if h.want[0] == "next" and h.want[1] + h.want[2] < H.CHUNK}
    assert inside >= {(w, n) for w in ("bare-then-part", "bare-then-line") for n in H.BARE_LEN if n + max(t, 1) < H.CHUNK}
    assert any(h.aim == "value-colons" for _, h in col) and col[-1][1].aim == "bare-then-end"
    # keys: the four keys, their near-misses and every schema name at the four byte alignments
    ks = aimed(S["keys"])
    got = {(h.aim, (a + h.pos) & 3) for a, h in ks}
    want = {(f"{w} {k.decode()}", r) for w in ("key", "near") for k in H.KEYS for r in q4}
    want |= {(f"schema {ty} {n}", r) for ty in H.TYPES for n in range(1, 21) for r in q4}
    want |= {(f"twins {k}", r) for k in (15, 16, 17) for r in q4} | {("utf-8", r) for r in q4} | {("schema long", r) for r in q4}
    assert got == want
    assert all(a % 4 == 0 for a in S["keys"].offsets)
    for k in H.KEYS:
        assert sum(1 for _, h in ks if h.aim == "near " + k.decode()) == 4 * len(H.near_misses(k)) and len(set(H.near_misses(k))) == 6
    # suffix: lengths 0, 1, 7, 8 and 9, every case of each at the four alignments of the compare
    lens = set()
    for name, sufs in (("suffix", H.SUFFIX), ("suffix9", H.SUFFIX9)):
        got = {(h.aim, (a + h.pos) & 3) for a, h in aimed(S[name])}
        assert got == {(f"{len(s)} {case}", r) for s in sufs.values() for case, _, _ in H.suffix_names(s) for r in q4}
        lens |= {len(s) for s in sufs.values()}
    assert lens == {0, 1, 7, 8, 9}
    # records: for every base & 3 the flip at pair 0, 1, 2, 5, one byte short of the limit, at it and one byte past it, the limit
    # being a part's first byte and the line's end; the pair counts of the copy-out
    rec = aimed(S["records"])
    assert {h.want[1:] for _, h in rec if h.aim == "flip"} == \
        {(o, m, d, w) for o in q4 for m in H.REC_M for d in (-1, 0, 1) for w in ("part", "end")}
    assert {(h.aim, a & 3) for a, h in rec if h.aim != "flip"} == \
        {(f"count {n} {w}", o) for n in H.PAIR_COUNTS for w in ("roomy", "tiny") for o in q4}
    # value-end: every case followed by a line that would extend it, one as the batch's last line
    ve = aimed(S["value-end"])
    assert {h.aim for _, h in ve} == {c[0] for c in H.value_end_cases()} and ve[-1][1].want == ("follows", b"")
    assert sum(1 for _, h in ve if h.want[1]) == 4 * len(H.value_end_cases())
    # head-end: for every o0 & 15 the head's end at every byte of every object, one byte before and one behind
    he = aimed(S["head-end"])
    got = {(h.aim, h.want[1], a & 15) for a, h in he if h.want[0] == "head"}
    want = {(f"{name} {w}", d, r) for name, _, size, _ in H.head_objects() for w in ("+", "last") for d in range(-1, size + 2) for r in al16}
    want |= {("tab", d, r) for d in (0, 1) for r in al16}
    assert got == want
    assert {(h.want[1], a & 15) for a, h in he if h.aim == "boundary"} == {(v, r) for v in range(510, 515) for r in al16}
    assert {v for v in range(510, 515)} == set(range(H.HEAD - 2, H.HEAD + 3))
    # behind-head
    bh = aimed(S["behind-head"])
    assert {(h.want[1], a & 15) for a, h in bh if h.aim == "rest-tab"} == {(r, al) for r in H.REST_AT for al in (0, 1, 15)}
    assert set(H.REST_AT) == {0, 1, 15, 16, H.ROW - 1, H.ROW, H.ROW + 1, 2 * H.ROW - 1, 2 * H.ROW}
    assert {((len(h.line) - H.head_at(a)) & 3, h.want[1]) for a, h in bh if h.aim == "last-four"} == {(m, j) for m in q4 for j in (1, 2, 3, 4)}
    assert {(len(h.line) & 3, h.want[1]) for a, h in bh if h.aim == "last-four"} == {(m, j) for m in q4 for j in (1, 2, 3, 4)}
    assert {(len(h.line)) for _, h in bh if h.aim == "name-limit"} == set(H.BIG)
    rows = [-(-(len(h.line) - H.head_at(a)) // H.ROW) for a, h in bh if h.aim == "rows"]
    assert len(rows) >= 64 and min(rows) >= 3 and sum(rows[:64]) > 3 * 64
    assert sum(1 for _, h in bh if h.aim == "tab-behind-end") == 8


# ---- b) -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("framing", FRAMINGS, ids=IDS)
def test_the_oracle_gives_every_line_what_it_was_built_to_give(oracle, framing):
    n_ok = n_err = 0
    for s in H.streams(framing):
        data, offsets = synth.pack(s.lines())
        blob, offs = oracle.decode_batch(LTSV, data, offsets, s.config)
        assert len(offs) == len(s.ln) + 1
        for i, h in enumerate(s.ln):
            got = parse_canonical(blob[int(offs[i]):int(offs[i + 1])].tobytes())
            ctx = f"{s.name} line {i} [{h.cls} {h.aim} pos {h.pos} want {h.want}]: {h.line[:160]!r}"
            if isinstance(h.exp, str):
                assert isinstance(got, DecodeError) and str(got) == h.exp, f"{ctx}\n  built  {h.exp!r}\n  oracle {got!r}"
                n_err += 1
            else:
                assert not isinstance(got, DecodeError), f"{ctx}\n  oracle {got!r}"
                assert got == h.exp, f"{ctx}\n  built  {h.exp!r}\n  oracle {got!r}"[:3000]
                n_ok += 1
    print({"ok": n_ok, "intended errors": n_err})
    assert n_ok > 8000 and n_err > 50


# ---- c) -----------------------------------------------------------------------------------------------------------------------------
def test_the_geometry_is_the_one_in_the_sources():
    ltsv = (CSRC / "fg_ltsv.hip").read_text()
    pipe = (CSRC / "fg_pipeline.hpp").read_text()

    def one(pattern: str, text: str) -> int:
        m = re.findall(pattern, text)
        assert len(set(m)) == 1, (pattern, m)
        return int(m[0], 0)

    assert one(r"static constexpr uint32_t kHeadBytes = (\d+);", ltsv) == H.HEAD
    # ... which is what geometry_head stages, alignment slack included, and tlen the bytes of the line among them
    assert "struct head_cap<F, decltype((void)F::kHeadBytes)> { static constexpr uint32_t value = F::kHeadBytes; };" in pipe
    assert "const uint64_t want = (o1 - o0) + (o0 & 15ull);" in pipe and "want >= head_cap<F>::value ? head_cap<F>::value" in pipe
    assert "const uint32_t al = (uint32_t)(o0 & 15ull)" in pipe and "c.tlen = st == 0u ? 0u : (st - al < len ? st - al : len);" in pipe
    assert one(r"constexpr uint32_t kHeadCap = (\d+);", pipe) >= H.HEAD and H.HEAD % H.CHUNK == 0
    # tab_behind_head: rows of 1 << 10 bytes
    assert 1 << one(r"\(rem \+ 1023u\) >> (\d+);", ltsv) == H.ROW
    assert 1 << one(r"const uint32_t off = \(row - kfirst\) << (\d+);", ltsv) == H.ROW
    # next_tab: a 64-bit window, refilled when the search is 64 or more bits past its first
    assert "tabw = wv::window64(T.bm, base + from);" in ltsv
    assert one(r"if \(off < (\d+)u\) \{", ltsv) == H.TAB_WINDOW and one(r"from = tw0 \+ (\d+)u;", ltsv) == H.TAB_WINDOW
    # the ':' window and the records
    assert one(r"const uint32_t in_part = plen >= (\d+)u \? 0xFFFFu", ltsv) == H.CHUNK
    assert one(r"\} else if \(plen > (\d+)u\) \{", ltsv) == H.CHUNK
    assert "uint32_t wpos = (base + 3u) & ~3u;" in ltsv and H.RECORD_ALIGN == 4
    assert one(r"if \(wpos \+ (\d+)u <= base \+ \(more \? nps : len\)\)", ltsv) == H.RECORD
    assert one(r"wpos \+= (\d+)u;", ltsv) == H.RECORD
    assert one(r"const bool name_fits = len < (\d+)u;", ltsv) == H.NAME_LIMIT


# ---- d) -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("framing", FRAMINGS, ids=IDS)
def test_records_class_straddles_the_fit_condition(framing):
    s = by_name(framing)["records"]
    changed, at_limit = set(), set()
    for i, (a, h) in enumerate(zip(s.offsets, s.ln)):
        if h.aim != "flip":
            continue
        fits, strict = H.first_unfit(h.line, a), H.first_unfit(h.line, a, strict=True)
        m, d = h.want[2], h.want[3]
        if fits != strict:
            changed.add(i)
            assert strict == m and (fits is None or fits > m)  # pair m fits with `<=` and would not with `<`
        if d == 0:
            at_limit.add(i)
        assert (fits == m) == (d == 1) and (strict == m) == (d >= 0)
    assert changed == at_limit and len(changed) == 4 * len(H.REC_M) * 2
