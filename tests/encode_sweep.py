"""Value lists for the encoder sweeps (timestamps, typed pair values, priorities) and a plain reference of the number and date text the
encoders print, in Python integers and `decimal`.

The reference functions restate the reference's encoder sources, not the kernels' headers:
  rfc5424_encoder.rs:43-53  `((record.ts * 1000.0) as i128) * 1_000_000` (release build: the cast saturates, NaN -> 0, the product wraps),
                            OffsetDateTime::from_unix_timestamp_nanos (time 0.3: years -9999 ..= 9999, else "Failed to parse date"),
                            format(&Rfc3339) (years 0 ..= 9999, else "Failed to parse date as Rfc3339 format"; the subsecond part is the
                            nanoseconds without their trailing zeros, absent when zero)
  rfc3164_encoder.rs:50-63  OffsetDateTime::from_unix_timestamp(record.ts as i64), "[month repr:short]  [day padding:none] [hour]:[minute]:[second] "
  ltsv_encoder.rs:84,101    f64::to_string() = Display: the shortest digits that read back, positional, no exponent, no ".0"

The lists are deterministic (seeded random.Random).  QUALIFIED pins n and a hash of each list: the CPU test checks the coverage conditions on
exactly these lists, the GPU tests check that the values they patched into the tables are these lists."""
import hashlib
import math
import random
import struct
from bisect import bisect_right
from decimal import Decimal

MIN_UNIX, MAX_UNIX = -377705116800, 253402300799    # -9999-01-01T00:00:00 .. 9999-12-31T23:59:59
YEAR0_UNIX = -62167219200                           # 0000-01-01T00:00:00
E_DATE, E_FORMAT, E_3164 = "Failed to parse date", "Failed to parse date as Rfc3339 format", "Failed to parse unix timestamp in RFC3164 encoder"
MONTHS = ["Jan", "Feb", "Mar", "Apr", "May", "Jun", "Jul", "Aug", "Sep", "Oct", "Nov", "Dec"]


def bits_f64(b: int) -> float:
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def f64_bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


# ---- the plain reference ------------------------------------------------------------------------------------------------------------
def is_leap(y: int) -> bool:
    return y % 4 == 0 and (y % 100 != 0 or y % 400 == 0)


def month_lengths(y: int):
    return [31, 29 if is_leap(y) else 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31]


# first day of each year of one 400-year cycle, counted from 1 January of the cycle's first year (year 0 is a leap year)
_CYCLE = [0]
for _y in range(400):
    _CYCLE.append(_CYCLE[-1] + (366 if is_leap(_y) else 365))
assert _CYCLE[400] == 146097
DAYS_0000_TO_1970 = 4 * 146097 + _CYCLE[370]  # 1970 = 4 * 400 + 370


def civil(secs: int):
    """proleptic Gregorian (year, month, day, hour, minute, second) of a unix time"""
    days, sod = divmod(secs, 86400)
    cyc, d = divmod(days + DAYS_0000_TO_1970, 146097)
    yy = bisect_right(_CYCLE, d) - 1
    d -= _CYCLE[yy]
    y = 400 * cyc + yy
    m = 0
    for ml in month_lengths(y):
        if d < ml:
            break
        d -= ml
        m += 1
    return y, m + 1, d + 1, sod // 3600, sod // 60 % 60, sod % 60


def unix_of(y, mo, d, hh=0, mi=0, ss=0) -> int:
    cyc, yy = divmod(y, 400)
    days = cyc * 146097 + _CYCLE[yy] + sum(month_lengths(y)[:mo - 1]) + d - 1 - DAYS_0000_TO_1970
    return days * 86400 + hh * 3600 + mi * 60 + ss


def saturating_cast(x: float, bits: int) -> int:
    """Rust `x as iN`: truncates toward zero, saturates, NaN -> 0"""
    if x != x:
        return 0
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    if x == math.inf:
        return hi
    if x == -math.inf:
        return lo
    return max(lo, min(hi, int(x)))


def rfc5424_ns(ts: float) -> int:
    """((ts * 1000.0) as i128) * 1_000_000, wrapped to 128 bits"""
    p = (saturating_cast(ts * 1000.0, 128) * 1_000_000) & ((1 << 128) - 1)
    return p - (1 << 128) if p >> 127 else p


def rfc5424_date(ts: float) -> str:
    """the RFC5424 encoder's timestamp text ("2015-08-06T11:15:24.638Z") or its error string"""
    secs, nanos = divmod(rfc5424_ns(ts), 1_000_000_000)
    if not MIN_UNIX <= secs <= MAX_UNIX:
        return E_DATE
    y, mo, d, hh, mi, ss = civil(secs)
    if not 0 <= y <= 9999:
        return E_FORMAT
    frac = ("." + "%09d" % nanos).rstrip("0") if nanos else ""
    return "%04d-%02d-%02dT%02d:%02d:%02d%sZ" % (y, mo, d, hh, mi, ss, frac)


def rfc3164_secs(ts: float):
    """`record.ts as i64` when from_unix_timestamp accepts it, else the encoder's error string"""
    secs = saturating_cast(ts, 64)
    return secs if MIN_UNIX <= secs <= MAX_UNIX else E_3164


def rfc3164_date(ts: float) -> str:
    """the RFC3164 encoder's timestamp text with its trailing space ("Aug  6 11:15:24 ") or its error string"""
    secs = rfc3164_secs(ts)
    if isinstance(secs, str):
        return secs
    _, mo, d, hh, mi, ss = civil(secs)
    return "%s  %d %02d:%02d:%02d " % (MONTHS[mo - 1], d, hh, mi, ss)


def rust_display(x: float) -> str:
    """Rust's `{}` of an f64: repr() has the shortest digits that read back; Decimal spreads them out positionally"""
    if x != x:
        return "NaN"
    if x in (math.inf, -math.inf):
        return "inf" if x > 0 else "-inf"
    s = format(Decimal(repr(x)), "f")
    if "." in s:
        s = s.rstrip("0").rstrip(".")
    return s


# ---- the value lists ----------------------------------------------------------------------------------------------------------------
# every stamp test_emit_cpu.py::rrecord lists
RRECORD_STAMPS = [0.0, -0.5, 1438790025.637824, 1438859724.0, 253402300799.9, 253402300800.0, -62167219200.5, -62167219201.0,
                  -377705116800.0, -377705116801.0, 1e25, -1e25, 1e300, math.nan, math.inf, -math.inf, 9.3e18, -9.3e18]
# (numerator, digits) of the fractions added to a whole second: 0, 1, 3, 6, 9 digits and the neighbours of a millisecond step
# (`ts * 1000.0` truncates: .0005 and .9995 sit half-way, .999999999 just below the next second)
FRACTIONS = [(0, 0), (5, 1), (7, 1), (638, 3), (1, 3), (999, 3), (637824, 6), (999999, 6), (123456789, 9), (999999999, 9), (1, 9),
             (5, 4), (9995, 4), (4999, 7), (1000001, 9)]
WRAP_SEARCH_EXPONENTS = range(54, 70)


def _with_fraction(sec: int, num: int, digits: int) -> float:
    """sec + num / 10^digits, correctly rounded (the value whose decimal text a sender would have written)"""
    return float(Decimal(sec) + Decimal(num).scaleb(-digits))


def wrapped_in_range():
    """Stamps whose `* 1_000_000` WRAPS and still lands inside the date range -- the only way to a nanosecond field that is no multiple
    of a millisecond.  x = ts * 1000.0 = m * 2^e (m < 2^53) gives x * 10^6 = (m * 15625 mod 2^(122-e)) * 2^(e+6) modulo 2^128, which is
    in range only when the left factor is a small j: m = j * 15625^-1 mod 2^(122-e), and that has to fit 53 bits.  The search is
    exhaustive over e and j; whatever it finds (possibly nothing) joins the list."""
    out = []
    for e in WRAP_SEARCH_EXPONENTS:
        mod = 1 << (122 - e)
        if mod <= 1:
            continue
        inv = pow(15625, -1, mod)
        step = 1 << (e + 6)
        jmax = (-MIN_UNIX * 10 ** 9) // step + 1
        for j in range(-jmax, jmax + 1):
            m = (j * inv) % mod
            if j == 0 or m == 0 or m >> 53:
                continue
            x = float(m) * 2.0 ** e
            for sign in (1.0, -1.0):
                for ts in (sign * x / 1000.0, math.nextafter(sign * x / 1000.0, math.inf), math.nextafter(sign * x / 1000.0, -math.inf)):
                    if ts * 1000.0 == sign * x and not rfc5424_date(ts).startswith("Failed to parse date") and ts not in out:
                        out.append(ts)
    return out


def _boundary_seconds():
    """whole seconds at which the calendar arithmetic can go wrong"""
    secs = []
    for y in (-1, 0, 1, 1969, 1970, 1971, 1999, 2000, 2001, 2038, 9999):
        secs += [unix_of(y, 1, 1) + d for d in (-2, -1, 0, 1, 2)]
    for y in (1900, 2000, 2024, 2100):  # 28 February .. 1 March: the last second of each day and the first of the next
        for mo, d in ((2, 28), (2, 29), (3, 1)) if is_leap(y) else ((2, 28), (3, 1)):
            secs += [unix_of(y, mo, d), unix_of(y, mo, d, 12, 34, 56), unix_of(y, mo, d, 23, 59, 59)]
    for y in (2024, 2023):              # each month end of one leap and one common year
        for mo in range(1, 13):
            secs += [unix_of(y, mo, month_lengths(y)[mo - 1], 23, 59, 59), unix_of(y, mo, month_lengths(y)[mo - 1], 23, 59, 59) + 1]
    secs += [2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32, -2 ** 31, -2 ** 31 - 1, MAX_UNIX, MAX_UNIX - 1, MIN_UNIX, MIN_UNIX + 1, YEAR0_UNIX, YEAR0_UNIX + 1]
    return secs


def timestamps(n: int):
    """n Record.ts values; at least 60 % lie inside [MIN_UNIX, MAX_UNIX]"""
    r = random.Random(5424)
    special = list(RRECORD_STAMPS)
    for lim in (MIN_UNIX, MAX_UNIX, YEAR0_UNIX):  # both range limits (and year 0, the RFC3339 limit) +-1 and +-0.001
        special += [float(lim + d) for d in (-1, 1)] + [_with_fraction(lim, s * 1, 3) for s in (-1, 1)]
    # the limits as the RFC3164 encoder sees them: `as i64` truncates toward zero, so the fractions just outside still pass
    special += [MIN_UNIX - 0.999, MIN_UNIX - 1.0, math.nextafter(MIN_UNIX - 1.0, 0.0), MAX_UNIX + 0.999, MAX_UNIX + 1.0, math.nextafter(MAX_UNIX + 1.0, 0.0)]
    special += [0.0, -0.0, 0.5, -0.5, 5e-324, -5e-324, 0.001, -0.001, 0.0009999999999999, -0.0009999999999999]
    for mag in (9.3e18, 1.7e35, 1.8e38, 1e300, 1.7976931348623157e308,
                2.0 ** 63, 2.0 ** 64, 2.0 ** 63 / 1000.0, 2.0 ** 64 / 1000.0, 2.0 ** 127 / 1000.0, 2.0 ** 126 / 1000.0, 2.0 ** 122 / 1000.0):
        for v in (mag, math.nextafter(mag, 0.0), math.nextafter(mag, math.inf)):
            special += [v, -v]
    special += [math.nan, bits_f64(0xFFF8000000000000), bits_f64(0x7FF8000000001234), bits_f64(0xFFF800DEADBEEF01), math.inf, -math.inf]
    special += wrapped_in_range()

    boundary = [_with_fraction(s, num, dig) for s in _boundary_seconds() for num, dig in FRACTIONS]
    n_rest = min(n, max(len(special), n * 30 // 100))                 # specials, then random bit patterns
    n_in = n - n_rest
    out = boundary[:n_in]
    while len(out) < n_in:
        k = len(out) % 8
        if k == 0:
            sec = r.randint(MIN_UNIX, MAX_UNIX)                       # the whole range: mostly negative years
        elif k in (1, 2):
            sec = r.randint(YEAR0_UNIX, MAX_UNIX)                     # every year the RFC5424 encoder prints
        elif k == 3:
            sec = r.randint(-2 ** 31, -1)                             # 1901 .. 1969: negative with a fraction
        else:
            sec = r.randint(0, 2 ** 32)                               # 1970 .. 2106
        num, dig = FRACTIONS[r.randrange(len(FRACTIONS))] if r.random() < 0.5 else (lambda d: (r.randrange(10 ** d), d))(r.choice([0, 1, 3, 6, 9]))
        if k >= 6:
            sec = sec % 10 ** r.randint(1, 8) * (1 if k == 6 else -1)  # few integer digits: all nine fraction digits survive in the f64
        out.append(_with_fraction(sec, num, dig))
    out += special[:n_rest]
    while len(out) < n:
        out.append(bits_f64(r.getrandbits(64)))
    return out


def f64_values(n: int):
    """n F64 pair values"""
    r = random.Random(64)
    out = [0.0, -0.0, 1.5, 123.456, 1e21, 1e-7, math.nan, math.inf, -math.inf, bits_f64(0x7FF8000000001234), bits_f64(0xFFF8000000000000)]  # rvalue's list
    for k in range(-323, 309):          # every power of ten and its two neighbours
        p = float("1e%d" % k)
        out += [p, math.nextafter(p, 0.0), math.nextafter(p, math.inf)]
    for k in range(-1074, 1024, 7):     # powers of two, the subnormal ones included
        out += [2.0 ** k, -(2.0 ** k)]
    out += [2.0 ** 53 - 1, 2.0 ** 53, 2.0 ** 53 + 2, -(2.0 ** 53) - 2, 2.0 ** 63, 2.0 ** 64, 5e-324, 2.2250738585072014e-308, 2.225073858507201e-308,
            1.7976931348623157e308, -1.7976931348623157e308, 0.1, 0.3, 1 / 3, 2 / 3, 9007199254740993.0, 1e15, 1e16, 1e17, 9999999999999998.0, 99999999999999984.0]
    for digits in range(1, 18):         # 1 .. 17 significant digits at several exponents
        for _ in range(12):
            m = r.randrange(10 ** (digits - 1), 10 ** digits)
            out.append(float("%de%d" % (m, r.choice([-digits, -digits + 3, 0, -3, 5, -12, 20, -25]))) * r.choice([1, -1]))
    while len(out) < n:
        k = len(out) % 3
        out.append(bits_f64(r.getrandbits(64)) if k == 0 else r.random() * 10.0 ** r.randint(-10, 25) if k == 1
                   else bits_f64(r.getrandbits(52)))  # (a subnormal)
    assert len(out) == n, "n is too small for the fixed part of the list"
    return out


_CHUNKS = sorted({0, 2 ** 64 - 1, 2 ** 63, 2 ** 63 - 1} | {10 ** k + d for k in range(0, 20) for d in (-1, 0, 1) if 0 <= 10 ** k + d < 2 ** 64})


def u64_values():
    """the chunk boundaries of test_integer_text_at_the_chunk_boundaries and 2 000 random values of every length"""
    r = random.Random(164)
    return _CHUNKS + [r.getrandbits(r.randint(1, 64)) for _ in range(2000)]


def i64_values():
    r = random.Random(163)
    fixed = sorted({-v for v in _CHUNKS if v <= 2 ** 63} | {v for v in _CHUNKS if v < 2 ** 63} | {-2 ** 63, 2 ** 63 - 1, -1})
    return fixed + [r.getrandbits(r.randint(1, 63)) * r.choice([1, -1]) for _ in range(2000)]


def pri_values():
    """(facility, severity): every facility 0 .. 31 and None x every severity 0 .. 7 and None"""
    return [(f, s) for f in list(range(32)) + [None] for s in list(range(8)) + [None]]


def sweep_hash(values) -> str:
    """hash of a value list: floats by their IEEE bits, integers as 128-bit two's complement, None as a marker"""
    h = hashlib.sha256()
    for v in values:
        for x in v if isinstance(v, tuple) else (v,):
            h.update(b"n" if x is None else b"f" + struct.pack("<d", x) if isinstance(x, float) else b"i" + (x & (1 << 128) - 1).to_bytes(16, "little"))
    return h.hexdigest()[:32]


N_TS, N_F64 = 12301, 6007   # no multiples of the wave size
# list -> (n, sweep_hash): what test_encode_sweep_cpu.py qualified and the GPU sweeps must be running
QUALIFIED = {
    "timestamps": (N_TS, "e788a123911cd244931dfab6ab2d9474"),
    "f64_values": (N_F64, "f515d7940afbd9223e165e2a7473675c"),
    "i64_values": (2116, "997a0f3a703e172affa50730352e8f7d"),
    "u64_values": (2063, "63d9225d8bacf14acce1ee2ca250e8fa"),
    "pri_values": (297, "42fb50257f603c71350b53b388a304f0"),
}


def qualified(name: str):
    """the qualified list `name`, checked against its pinned length and hash"""
    n, want = QUALIFIED[name]
    vals = {"timestamps": lambda: timestamps(N_TS), "f64_values": lambda: f64_values(N_F64), "i64_values": i64_values, "u64_values": u64_values,
            "pri_values": pri_values}[name]()
    assert len(vals) == n and sweep_hash(vals) == want, (name, len(vals), sweep_hash(vals))
    return vals
