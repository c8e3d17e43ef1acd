"""CPU: qualify the sweeps the GPU tests run (tests/test_gpu_encode_sweep.py).  Both sides of a device comparison must not be the same
author's recollection, so the oracle's date and number text is pinned first against a plain reference (encode_sweep.py: Python integers
and `decimal`, written from the reference's encoder sources) and against `datetime`; then the host build of the emitters is compared with
the oracle on the same lists; then the coverage conditions are asserted on the oracle alone, so that the GPU tests cannot pass by
formatting nothing."""
import datetime
import math

import pytest

import encode_sweep as S
import oracle_binding as OB
from test_emit_cpu import GELF, LTSV, RFC5424, emit  # noqa: F401  (emit: the fixture)
from test_encoder_cpu import canonical


@pytest.fixture(scope="module")
def stamps():
    return S.qualified("timestamps")


@pytest.fixture(scope="module")
def dates(oracle, stamps):
    """per stamp: what the oracle's RFC5424 / RFC3164 / LTSV encoders give for the minimal Record"""
    out = []
    for ts in stamps:
        cb = canonical(ts=ts, hostname="h")
        out.append(tuple(oracle.encode(e, cb) for e in (OB.ENC_RFC5424, OB.ENC_RFC3164, OB.ENC_LTSV)))
    return out


def text(w):
    return w if isinstance(w, str) else w.decode()


def test_every_list_is_the_qualified_one():
    for name, (n, _) in S.QUALIFIED.items():
        assert len(S.qualified(name)) == n
    assert S.N_TS % 64 and S.N_F64 % 64
    ts = S.timestamps(S.N_TS)
    assert sum(1 for t in ts if S.MIN_UNIX <= t <= S.MAX_UNIX) >= 0.6 * len(ts)
    bits = {S.f64_bits(t) for t in ts}
    for t in S.RRECORD_STAMPS + [0.0, -0.0, 5e-324, -5e-324, 1e300, -1e300, 1.7976931348623157e308, S.MIN_UNIX - 0.001, S.MAX_UNIX + 0.001,
                                 float(S.MIN_UNIX - 1), float(S.MAX_UNIX + 1), math.inf, -math.inf]:
        assert S.f64_bits(t) in bits, t
    assert sum(1 for t in ts if t != t) >= 4 and {S.f64_bits(t) >> 63 for t in ts if t != t} == {0, 1}
    vals = S.f64_values(S.N_F64)
    vb = {S.f64_bits(v) for v in vals}
    for k in range(-323, 309):
        p = float("1e%d" % k)
        assert {S.f64_bits(p), S.f64_bits(math.nextafter(p, 0.0)), S.f64_bits(math.nextafter(p, math.inf))} <= vb, k
    assert len(S.pri_values()) == 33 * 9


def test_oracle_dates_equal_the_plain_reference(stamps, dates):
    for ts, (w5424, w3164, wltsv) in zip(stamps, dates):
        d = S.rfc5424_date(ts)
        assert text(w5424) == (d if d.startswith("Failed") else "<13>1 %s h - - - " % d), (ts.hex(), w5424, d)
        d = S.rfc3164_date(ts)
        assert text(w3164) == (d if d.startswith("Failed") else d + "h "), (ts.hex(), w3164, d)
        assert text(wltsv) == "host:h\ttime:" + S.rust_display(ts), (ts.hex(), wltsv)


def test_plain_reference_equals_datetime_in_years_1_to_9999(stamps):
    epoch = datetime.datetime(1970, 1, 1)
    lo, hi = S.unix_of(1, 1, 1), S.MAX_UNIX
    n = 0
    for ts in stamps:
        ns = S.rfc5424_ns(ts)
        secs, nanos = divmod(ns, 10 ** 9)
        if lo <= secs <= hi:
            dt = epoch + datetime.timedelta(seconds=secs)
            frac = ("." + "%09d" % nanos).rstrip("0") if nanos else ""
            assert S.rfc5424_date(ts) == dt.strftime("%%04d-%m-%dT%H:%M:%S") % dt.year + frac + "Z", ts.hex()
            n += 1
        s = S.rfc3164_secs(ts)
        if not isinstance(s, str) and lo <= s <= hi:
            dt = epoch + datetime.timedelta(seconds=s)
            assert S.rfc3164_date(ts) == "%s  %d %s " % (S.MONTHS[dt.month - 1], dt.day, dt.strftime("%H:%M:%S")), ts.hex()
    assert n > 0.5 * len(stamps)
    # and the calendar arithmetic on its own: the first and the last day of every month of years 1 .. 9999, and every 97th day
    for y in range(1, 10000):
        for mo in range(1, 13):
            first = (datetime.date(y, mo, 1) - datetime.date(1970, 1, 1)).days
            assert S.civil(first * 86400)[:3] == (y, mo, 1) and S.unix_of(y, mo, 1) == first * 86400
            prev = datetime.date.fromordinal(first + 719163 - 1) if (y, mo) != (1, 1) else None
            assert prev is None or S.civil(first * 86400 - 1) == (prev.year, prev.month, prev.day, 23, 59, 59)
    for days in range(lo // 86400, hi // 86400 + 1, 97):
        d = datetime.date.fromordinal(days + 719163)
        assert S.civil(days * 86400 + 86399)[:3] == (d.year, d.month, d.day)


def test_oracle_number_text(oracle):
    """Display of F64 pair values against the plain reference (LTSV and the RFC5424 SD), the integers against str(); dtoa (Grisu2: no
    independent reference for its digit choice, the reference's vectors pin it elsewhere) must read back"""
    vals = S.qualified("f64_values") + S.qualified("timestamps")
    for v in vals:
        assert oracle.rust_display(v) == S.rust_display(v), v.hex()
        if math.isfinite(v):
            assert float(oracle.dtoa(v)) == v and S.f64_bits(float(oracle.dtoa(v))) == S.f64_bits(v), (v.hex(), oracle.dtoa(v))
    f = S.qualified("f64_values")
    for i in range(0, len(f), 8):
        pairs = [("_k%d" % j, (2, v)) for j, v in enumerate(f[i:i + 8])]
        cb = canonical(ts=1.5, hostname="h", sd=[("id", pairs)])
        want = "".join("k%d:%s\t" % (j, S.rust_display(v)) for j, v in enumerate(f[i:i + 8])) + "host:h\ttime:1.5"
        assert oracle.encode(OB.ENC_LTSV, cb).decode() == want
        want = "<13>1 1970-01-01T00:00:01.5Z h - - [id" + "".join(' k%d="%s"' % (j, S.rust_display(v)) for j, v in enumerate(f[i:i + 8])) + "] "
        assert oracle.encode(OB.ENC_RFC5424, cb).decode() == want
    iv, uv = S.qualified("i64_values"), S.qualified("u64_values")
    assert min(iv) == -2 ** 63 and max(iv) == 2 ** 63 - 1 and max(uv) == 2 ** 64 - 1 and min(uv) == 0
    for ty, ints in ((3, iv), (4, uv)):
        for i in range(0, len(ints), 8):
            cb = canonical(ts=1.5, hostname="h", sd=[(None, [("_k%d" % j, (ty, v)) for j, v in enumerate(ints[i:i + 8])])])
            assert oracle.encode(OB.ENC_LTSV, cb).decode() == "".join("k%d:%d\t" % (j, v) for j, v in enumerate(ints[i:i + 8])) + "host:h\ttime:1.5"
            assert oracle.encode(OB.ENC_GELF, cb).decode() == ("{" + "".join('"_k%d":%d,' % (j, v) for j, v in enumerate(ints[i:i + 8]))
                                                               + '"host":"h","short_message":"-","timestamp":1.5,"version":"1.1"}')
    for fac, sev in S.qualified("pri_values"):
        cb = canonical(ts=1.5, hostname="h", facility=fac, severity=sev)
        pri = "<13>" if fac is None or sev is None else "<%d>" % (fac * 8 + sev)
        assert oracle.encode(OB.ENC_RFC5424, cb).decode() == pri + "1 1970-01-01T00:00:01.5Z h - - - "
        assert oracle.encode(OB.ENC_RFC3164, cb).decode() == (pri if pri != "<13>" or (fac, sev) == (1, 5) else "") + "Jan  1 00:00:01 h "


ENCODERS = [OB.ENC_GELF, OB.ENC_LTSV, OB.ENC_RFC5424, OB.ENC_RFC3164]


@pytest.mark.parametrize("src", [RFC5424, LTSV, GELF], ids=["src_rfc5424", "src_ltsv", "src_gelf"])
def test_host_build_equals_oracle_on_the_timestamps(emit, oracle, stamps, src):  # noqa: F811
    for i, ts in enumerate(stamps):
        cb = canonical(ts=ts, hostname="h", facility=i % 24, severity=i % 8, msg="m")
        for enc in ENCODERS:
            merger = 3 if (i + enc) % 3 == 0 else 0  # syslen: the length prefix grows with the Display text
            assert emit(enc, merger, src, cb, variant=i & 1, seed=i) == oracle.encode(enc, cb, merger), (ts.hex(), enc, merger)


@pytest.mark.parametrize("src", [LTSV, GELF], ids=["src_ltsv", "src_gelf"])
def test_host_build_equals_oracle_on_the_typed_values(emit, oracle, src):  # noqa: F811
    f, iv, uv, pri = (S.qualified(k) for k in ("f64_values", "i64_values", "u64_values", "pri_values"))
    for sort_slots in (32, 8):  # the 8-slot ranking scratch of batches with few pairs per line
        emit.set_sort_slots(sort_slots)
        try:
            step = 16 if sort_slots == 32 else 5
            for i in range(0, len(f), step):
                pairs = [("_f%02d" % j, (2, v)) for j, v in enumerate(f[i:i + step])]
                pairs += [("_i%02d" % j, (3, iv[(i + j) % len(iv)])) for j in range(step // 4)] + [("_u%02d" % j, (4, uv[(i + j) % len(uv)])) for j in range(step // 4)]
                pairs += [("_b", (1, i % 2 == 0)), ("_n", (5, None))]
                fac, sev = pri[(i // step) % len(pri)]
                cb = canonical(ts=f[i], hostname="h", facility=fac, severity=sev, msg="m", sd=[(None, pairs)])
                for enc in ENCODERS:
                    assert emit(enc, 3, src, cb, variant=i & 1, seed=i) == oracle.encode(enc, cb, 3), (i, enc, [v.hex() for v in f[i:i + step]])
        finally:
            emit.set_sort_slots(32)
    for k in range(0, max(len(iv), len(uv)), 8):
        pairs = [("_i%d" % j, (3, v)) for j, v in enumerate(iv[k:k + 8])] + [("_u%d" % j, (4, v)) for j, v in enumerate(uv[k:k + 8])]
        cb = canonical(ts=1.5, hostname="h", msg="m", sd=[(None, pairs)])
        for enc in ENCODERS:
            assert emit(enc, 0, src, cb) == oracle.encode(enc, cb, 0), (enc, iv[k:k + 8], uv[k:k + 8])


def test_coverage_conditions(stamps, dates):
    """asserted on the oracle alone: what the GPU sweep is worth"""
    n = len(stamps)
    ok5424 = [text(d[0]) for d in dates if isinstance(d[0], bytes)]
    ok3164 = [d[1] for d in dates if isinstance(d[1], bytes)]
    assert len(ok5424) >= 0.5 * n and len(ok3164) >= 0.5 * n
    for k, err in ((0, S.E_DATE), (0, S.E_FORMAT), (1, S.E_3164)):
        assert sum(1 for d in dates if d[k] == err) >= 20, err
    assert sum(1 for t in stamps if t < 0 and math.isfinite(t) and t != int(t)) >= 100
    assert sum(1 for t, d in zip(stamps, dates) if t < 0 and isinstance(d[0], bytes) and b"." in d[0]) >= 100  # ... that the date encoder prints
    # Fraction digits after trailing-zero removal.  In the RFC5424 date the nanoseconds are `(ts * 1000.0) as i128 * 1_000_000`: a multiple
    # of a millisecond unless the product wraps, and no f64 wraps into the date range (test_no_stamp_wraps_into_the_date_range), so three
    # digits are the longest fraction that encoder can print; all nine digits occur in the Display text of the same stamps (LTSV `time:`).
    digits5424 = [len(t.split(" ")[1].split(".")[1]) - 1 if "." in t.split(" ")[1] else 0 for t in ok5424]
    assert all(sum(1 for d in digits5424 if d == k) >= 50 for k in (0, 1, 2, 3)) and max(digits5424) == 3
    display = [text(d[2]).split("time:")[1] for d in dates]
    assert sum(1 for t in display if "." in t and len(t.split(".")[1]) == 9) >= 50
    assert sum(1 for t in display if len(t) >= 300) >= 20      # the syslen prefix crosses 1000 only with these
    # calendar edges that must be among the stamps the encoders print
    printed = {t.split(" ")[1][:10] for t in ok5424}
    assert {"0000-01-01", "0000-12-31", "0001-01-01", "1969-12-31", "1970-01-01", "1900-02-28", "1900-03-01", "2000-02-29", "2024-02-29",
            "2100-02-28", "2100-03-01", "2038-01-19", "9999-12-31", "9999-01-01", "2023-02-28", "2024-12-31"} <= printed


def test_no_stamp_wraps_into_the_date_range():
    """the exhaustive search for an f64 whose `* 1_000_000` wraps around 2^128 and lands inside years -9999 .. 9999: there is none, so
    sub-millisecond digits cannot come out of the RFC5424 encoder.  (If the search ever finds one, timestamps() includes it.)"""
    assert S.wrapped_in_range() == []
    # what does come out past 2^127: the saturated cast times 10^6 wraps to -10^6 ns resp. 0
    assert S.rfc5424_date(1e300) == "1969-12-31T23:59:59.999Z" and S.rfc5424_date(-1e300) == "1970-01-01T00:00:00Z"
    assert S.rfc5424_date(2.0 ** 126 / 1000.0) == "1970-01-01T00:00:00Z"


def test_capnp_input_encoder_corpus_still_encodes(oracle):
    """test_gpu_capnp_in.py::encoder_corpus draws its timestamps from timestamps(): with the reader model, more than 100 of its Records
    must still encode under every text encoder (what the GPU test asserts as n_ok > 100)"""
    import capnp_read_model as M
    from test_gpu_capnp_in import NOW, canonical_of, encoder_corpus

    models = [M.handle_message(m) for m in encoder_corpus()]
    stamps = {S.f64_bits(w[1].ts) for w in models if w[0] == "ok"}
    assert len(stamps) > 100
    for enc in ENCODERS + [OB.ENC_PASSTHROUGH]:
        n_ok = sum(1 for w in models if w[0] == "ok" and isinstance(oracle.encode(enc, canonical_of(w[1]), 0, now_ts=NOW), bytes))
        assert n_ok > 100, (enc, n_ok)
