"""GPU: the encoders' number and date arithmetic, swept on the device.  The device compile of fg_dtoa.hpp / fg_shortest.hpp / fg_emit.hpp
takes other branches than the g++ host build the CPU suite checks (__umul64hi for the 128-bit products, __clzll, the byte-permute funnel,
compiler-expanded 64-bit division and f64 <-> integer conversions).  Each test decodes a small base batch, overwrites `ts`, `meta` or
`ent_val` of the decode table in HBM (tests/table_patch.py) and compares every encoder's bytes, offsets and status per row with
oracle.encode() of the Record with the same values substituted -- byte-exact, no tolerance.  The value lists are the ones
tests/test_encode_sweep_cpu.py qualified (same generator, same n, a hash of the list)."""
import math

import numpy as np
import pytest

import capnp_wire as W
import encode_sweep as S
import oracle_binding as OB
import table_patch as P
from table_patch import GELF, LTSV, RFC5424

pytestmark = pytest.mark.gpu
SRC = {"rfc5424": RFC5424, "ltsv": LTSV, "gelf": GELF}
NOW_TS_HASH = "c8e3acad7ec344b55314c46e60f604ac"  # of test_now_ts_sweep's 24 values, every one of them out of the qualified timestamps()
EXTRA = {"_a01": "replaced", "host": "forced", "Zeta": "capital first", "_q": "x\"y\\z\n\t:1", "_f00_f64": "shadow"}


def encoder(name, merger, extra=None, prepend=None):
    from flowgger_amd import GelfEncoder, LTSVEncoder, RFC3164Encoder, RFC5424Encoder
    cls, oenc, key = {"gelf": (GelfEncoder, OB.ENC_GELF, "gelf_extra"), "ltsv": (LTSVEncoder, OB.ENC_LTSV, "ltsv_extra"),
                      "rfc5424": (RFC5424Encoder, OB.ENC_RFC5424, None), "rfc3164": (RFC3164Encoder, OB.ENC_RFC3164, None)}[name]
    assert extra is None or key
    return cls({"output": {key: extra}} if extra else None, merger=merger, prepend=prepend), oenc


@pytest.mark.parametrize("src", ["rfc5424", "ltsv", "gelf"])
@pytest.mark.parametrize("enc", ["gelf", "ltsv", "rfc5424", "rfc3164"])
def test_timestamp_sweep(oracle, src, enc):
    """`ts` of every row <- timestamps(): Grisu2 (GELF "timestamp"), Display (LTSV time:), the RFC5424 date (saturating i128 cast, wrapping
    product, long division, calendar, fraction cut) and the RFC3164 date; rows whose date fails write nothing and carry the oracle's error"""
    stamps = S.qualified("timestamps")
    batch = P.base_batch(SRC[src], len(stamps), 2, oracle)
    recs, canon = P.patch(batch, ts=stamps)
    assert len(recs) == S.QUALIFIED["timestamps"][0] and S.sweep_hash([r.ts for r in recs]) == S.QUALIFIED["timestamps"][1]
    label = lambda i: "ts " + stamps[i].hex()  # noqa: E731
    seen = set()
    for merger in ("none", "syslen"):  # the length prefix crosses 10 / 100 / 1000 as the Display texts grow past 300 bytes
        prepend = "2026-09-23T10:11Z " if enc == "rfc3164" and merger == "syslen" else None
        e, oenc = encoder(enc, merger, prepend=prepend)
        expected = P.expected_stream(oracle, oenc, canon, merger, prepend=prepend)
        P.run_and_check(batch, e, expected, label)
        seen |= set(expected[2])
        if merger == "syslen":
            P.run_and_check(batch, e, expected, label, use_async=True)
    assert seen == {"gelf": {None}, "ltsv": {None}, "rfc5424": {None, S.E_DATE, S.E_FORMAT}, "rfc3164": {None, S.E_3164}}[enc]


def test_timestamp_sweep_capnp_encoder(oracle):
    """the same stamps through the Cap'n Proto encoder: the raw f64, the only encoder through which a NaN's sign and payload must survive"""
    import torch

    from flowgger_amd import CapnpEncoder
    from test_gpu_capnp import first_bad, framed
    stamps = S.qualified("timestamps")
    batch = P.base_batch(GELF, len(stamps), 2, oracle)
    recs, _ = P.patch(batch, ts=stamps)
    assert len(recs) == S.QUALIFIED["timestamps"][0] and S.sweep_hash([r.ts for r in recs]) == S.QUALIFIED["timestamps"][1]
    msgs = [W.serialize(r, []) for r in recs]
    nan_rows = [i for i, t in enumerate(stamps) if t != t]
    assert len({S.f64_bits(stamps[i]) for i in nan_rows}) >= 4
    for i in nan_rows:
        assert S.f64_bits(W.parse(msgs[i])[0].ts) == S.f64_bits(stamps[i])  # the model itself keeps the bits
    for merger in (0, 3):
        enc = CapnpEncoder(None, merger=[None, "line", "nul", "syslen"][merger])
        d_out, d_off, d_st = enc.encode_device(batch.dec, batch.d_bytes, batch.d_offsets, batch.n, batch.tables, want_status=True)
        torch.cuda.synchronize()
        out, off = d_out.cpu().numpy().tobytes(), d_off.cpu().numpy().astype(np.uint64)
        want, woff = framed(msgs, np.zeros(len(msgs), np.uint8), merger)
        assert np.array_equal(off, woff) and out == want, first_bad(out, off, want, woff)
        assert not d_st.cpu().numpy().any()


@pytest.mark.parametrize("src", ["ltsv", "gelf"])
@pytest.mark.parametrize("enc", ["gelf", "ltsv", "rfc5424"])
def test_typed_value_sweep(oracle, src, enc):
    """`ent_val` of the F64 / I64 / U64 / BOOL entries <- the value lists: Grisu2 and the integer text in GELF members, Display in LTSV fields
    and the RFC5424 SD.  Rows of 6 and of 18 pairs: both have more than two entries per row on average, so under the GELF encoder both run
    the kernel with the 32-slot ranking scratch.  The 8-slot kernel is picked only for a table with at most 2 entries per row
    (fg_encode_device: ent_used <= 2 * n), and it is another translation unit that formats numbers too: rows of 2 pairs, F64 + I64 in one
    batch and U64 + BOOL in the next, put all three numeric lists through it."""
    lists = {P.T_F64: S.qualified("f64_values"), P.T_I64: S.qualified("i64_values"), P.T_U64: S.qualified("u64_values"),
             P.T_BOOL: [True, False, False, True, True]}
    names = {P.T_F64: "f64_values", P.T_I64: "i64_values", P.T_U64: "u64_values"}
    # rows: what consumes the longest list of the shape once (one F64 entry per group of six pairs), no multiple of the wave size
    shapes = [(S.N_F64, 6, 0, "none", None), (2011, 18, 0, "syslen", EXTRA if enc != "rfc5424" else None)]
    if enc == "gelf":  # (the only encoder with a ranking scratch)
        shapes += [(S.N_F64, 2, 0, "syslen", None), (2129, 2, 2, "none", None)]
    for n, pairs, first, merger, extra in shapes:
        batch = P.base_batch(SRC[src], n, pairs, oracle, first=first)
        assert (P.entries_reserved(batch) <= 2 * n) == (pairs == 2), "which ranking scratch this shape runs"
        present = {ty: vals for ty, vals in lists.items() if ty in batch.cycle}
        recs, canon = P.patch(batch, values=present)
        for ty, name in names.items():
            if ty in present:
                got = P.patched_values(recs, ty)
                assert len(got) >= len(lists[ty]) and S.sweep_hash(got[:len(lists[ty])]) == S.QUALIFIED[name][1], name

        def label(i, recs=recs, kinds=batch.cycle):
            return ", ".join(P.describe(v.value) for (_, v), t in zip(recs[i].sd[0].pairs, kinds) if t in names)
        e, oenc = encoder(enc, merger, extra=extra)
        expected = P.expected_stream(oracle, oenc, canon, merger, extra=extra)
        P.run_and_check(batch, e, expected, label)
        assert set(expected[2]) == {None}


@pytest.mark.parametrize("enc", ["gelf", "ltsv", "rfc5424", "rfc3164"])
def test_pri_sweep(oracle, enc):
    """facility / severity of `meta` <- every facility 0 .. 31 and None x every severity 0 .. 7 and None: pri() of the RFC5424 / RFC3164
    encoders, "level" of GELF, level: and facility: of LTSV"""
    pri = S.qualified("pri_values")
    meta = pri * 3  # 891 rows: fourteen waves, the last one partial
    batch = P.base_batch({"gelf": GELF, "ltsv": LTSV}.get(enc, RFC5424), len(meta), 2, oracle)
    recs, canon = P.patch(batch, meta=meta)
    assert S.sweep_hash([(r.facility, r.severity) for r in recs[:len(pri)]]) == S.QUALIFIED["pri_values"][1] and len(meta) % 64
    e, oenc = encoder(enc, "syslen")
    expected = P.expected_stream(oracle, oenc, canon, "syslen")
    P.run_and_check(batch, e, expected, lambda i: "facility %r severity %r" % meta[i])
    assert set(expected[2]) == {None}


def test_now_ts_sweep(oracle):
    """GELF rows without "timestamp" (FG_F_TS_NOW) take cfg.now_ts: 24 values, one encode call each"""
    stamps = S.qualified("timestamps")
    have = {S.f64_bits(t) for t in stamps}
    picks = [math.nan, S.bits_f64(0xFFF800DEADBEEF01), -0.5, float(S.MIN_UNIX), float(S.MAX_UNIX), 1e300, math.inf, -math.inf,
             1438790025.637824, 253402300799.9, -62167219200.5, -62167219201.0, 0.0, -0.0, 5e-324, 1e25, 9.3e18, S.MAX_UNIX + 1.0, S.MIN_UNIX - 1.0]
    picks += [t for t in stamps if -4e9 < t < 0 and t != int(t)][:24 - len(picks)]  # negative, with a fraction
    assert len(picks) == 24 and all(S.f64_bits(t) in have for t in picks), [t.hex() for t in picks if S.f64_bits(t) not in have]
    assert S.sweep_hash(picks) == NOW_TS_HASH
    batch = P.base_batch(GELF, 131, 2, oracle, timestamp=False)
    assert all(batch.ts_now)
    assert (P._column(batch.tables, "meta", np.uint32)[:batch.n] >> 24 & 1).all()  # FG_F_TS_NOW
    _, canon = P.patch(batch)
    for enc in ("gelf", "rfc5424"):
        e, oenc = encoder(enc, "syslen")
        for now in picks:
            expected = P.expected_stream(oracle, oenc, canon, "syslen", now_ts=now)
            P.run_and_check(batch, e, expected, lambda i, now=now: "now_ts " + now.hex(), now_ts=now)
