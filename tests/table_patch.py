"""GPU test harness: decode a small base batch, overwrite `ts`, `meta` and `ent_val` of the decode table IN HBM, and hand back the Records
with the same values substituted.  No parser sits between a chosen bit pattern and the emitters, which load those columns when they
encode: NaN, +-inf, -0.0 and stamps that no input format can carry reach every encoder this way.

The comparison helper runs an encoder on the patched table and checks bytes, offsets and status per row against oracle.encode()."""
import dataclasses
import struct

import numpy as np

import oracle_binding as OB
from flowgger_amd import synth
from flowgger_amd.record import Record, SDValue, _KINDS, parse_canonical
from gpu_util import device_path
from test_encoder_cpu import canonical

RFC5424, LTSV, GELF = 0, 1, 2
T_STRING, T_BOOL, T_F64, T_I64, T_U64, T_NULL, T_SDID = range(7)
# the pair types of one group of six, in line order
GELF_CYCLE = [T_F64, T_I64, T_U64, T_BOOL, T_NULL, T_STRING]
LTSV_CYCLE = [T_F64, T_I64, T_U64, T_BOOL, T_STRING, T_STRING]
MAX_PAIRS = 24
# synth.LTSV_CONFIG's suffixes with a schema wide enough for MAX_PAIRS distinct typed names
LTSV_SWEEP_CONFIG = {"input": {"ltsv_schema": {"%s%02d" % ("fiub"[k % 6], k): ["f64", "i64", "u64", "bool"][k % 6] for k in range(MAX_PAIRS) if k % 6 < 4},
                               "ltsv_suffixes": dict(synth.LTSV_CONFIG["input"]["ltsv_suffixes"])}}
MERGERS = {"none": OB.MERGE_NONE, "line": OB.MERGE_LINE, "nul": OB.MERGE_NUL, "syslen": OB.MERGE_SYSLEN}


def base_line(src, i, pairs, timestamp=True, first=0):
    """line i; pair k is position first + k of the cycle of six (its name carries that position)"""
    host = "host"[:1 + i % 4] + str(i % 10)
    msg = "message " + "abcdefghijklmnopqrstuvwxyz"[:i % 23]
    if src == GELF:
        text = ["1.5", "-3", "7", "true", "null", '"text"']
        kv = "".join(',"_a%02d":%s' % (p, text[p % 6]) for p in range(first, first + pairs))
        ts = ',"timestamp":1438790025.5' if timestamp else ""
        return ('{"version":"1.1","host":"%s","short_message":"%s"%s,"level":%d%s}' % (host, msg, ts, i % 8, kv)).encode()
    if src == LTSV:
        text = ["1.5", "-3", "7", "true", "text", "more"]
        kv = "".join("\t%s%02d:%s" % ("fiubst"[p % 6], p, text[p % 6]) for p in range(first, first + pairs))
        return ("time:1438790025.5\thost:%s\tmessage:%s\tlevel:%d%s" % (host, msg, i % 8, kv)).encode()
    sd = "[sd@%d %s]" % (i % 7, " ".join('k%02d="v%d"' % (k, k) for k in range(pairs))) if pairs else "-"
    return ("<%d>1 2015-08-05T15:53:45.637824Z %s app %d ID7 %s %s" % (i % 192, host, i, sd, msg)).encode()


@dataclasses.dataclass
class Batch:
    src: int
    n: int
    dec: object
    tables: object
    d_bytes: object
    d_offsets: object
    records: list      # the oracle's parsed Records of the base lines
    ts_now: list       # per row: the Record takes the caller's now_ts (GELF without "timestamp")
    cycle: list        # the entry types each row must hold
    host: dict = None  # ent_first / ent_count / ent_type on the host, copied once


def base_batch(src, n, pairs, orc, timestamp=True, first=0):
    """n short lines of one source format, decoded on the device; -> Batch.  first: where in the cycle of six pair types the rows' pairs
    start (rows of one or two pairs reach every numeric type that way)"""
    from flowgger_amd import GelfDecoder, LTSVDecoder, RFC5424Decoder

    assert first + pairs <= MAX_PAIRS
    lines = [base_line(src, i, pairs, timestamp, first) for i in range(n)]
    dec = {RFC5424: RFC5424Decoder, GELF: GelfDecoder, LTSV: lambda: LTSVDecoder(LTSV_SWEEP_CONFIG)}[src]()
    data, offsets = synth.pack(lines)
    tables, d_bytes, d_offsets = device_path(dec, data, offsets)
    blob, offs = orc.decode_batch(src, data, offsets, LTSV_SWEEP_CONFIG if src == LTSV else None)
    cb = [blob[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(n)]
    records = [parse_canonical(c, now=0.0) for c in cb]
    assert all(isinstance(r, Record) for r in records), next(r for r in records if not isinstance(r, Record))
    cycle = {GELF: GELF_CYCLE, LTSV: LTSV_CYCLE, RFC5424: [T_STRING] * 6}[src]
    want = ([T_SDID] if src == RFC5424 and pairs else []) + [cycle[p % 6] for p in range(first, first + pairs)]
    return Batch(src, n, dec, tables, d_bytes, d_offsets, records, [c[1] == 1 for c in cb], want)


def _column(tables, name, dtype):
    return tables.column(name).cpu().numpy().view(dtype).copy()


def _store(tables, name, arr):
    import torch

    col = tables.column(name)
    raw = torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8))
    assert raw.numel() == col.numel(), (name, raw.numel(), col.numel())
    col.copy_(raw)


def check_entry_types(batch):
    """the table rows and the oracle's Records hold exactly the entry types base_batch wrote: a decoder change cannot silently turn a
    typed sweep into a sweep of strings"""
    if batch.host is None:
        batch.host = {k: _column(batch.tables, k, dt) for k, dt in (("ent_first", np.uint32), ("ent_count", np.uint32), ("ent_type", np.uint8))}
    h = batch.host
    want = np.array(batch.cycle, np.uint8)
    assert (h["ent_count"][:batch.n] == len(want)).all(), ("ent_count", np.unique(h["ent_count"][:batch.n]), len(want))
    idx = h["ent_first"][:batch.n, None].astype(np.int64) + np.arange(len(want))[None, :]
    got = h["ent_type"][idx]
    assert (got == want[None, :]).all(), ("ent_type", got[np.flatnonzero((got != want[None, :]).any(axis=1))[0]].tolist(), want.tolist())
    pairs_want = [t for t in batch.cycle if t != T_SDID]
    for i, r in enumerate(batch.records):
        kinds = [_KINDS.index(v.kind) for e in (r.sd or []) for _, v in e.pairs]
        assert kinds == pairs_want, (i, kinds, pairs_want)
    return idx


def to_canonical(rec, ts_now=False):
    sd = None if rec.sd is None else [(e.sd_id, [(k, (_KINDS.index(v.kind), v.value)) for k, v in e.pairs]) for e in rec.sd]
    cb = canonical(rec.ts, rec.hostname, rec.facility, rec.severity, rec.appname, rec.procid, rec.msgid, rec.msg, rec.full_msg, sd)
    return cb[:1] + b"\x01" + cb[2:] if ts_now else cb


def patch(batch, ts=None, meta=None, values=None):
    """Overwrite table columns on the device and return (records, canonical bytes) with the same substitution.
    ts      n floats, written as their IEEE bits
    meta    n (facility, severity) with None = 0xFF; status and flags are kept
    values  {T_F64 / T_I64 / T_U64 / T_BOOL: list}: the entries of that type take the list's values in row order, then entry order,
            cyclically"""
    idx = check_entry_types(batch)
    n = batch.n
    recs = [dataclasses.replace(r) for r in batch.records]
    if ts is not None:
        assert len(ts) == n
        _store(batch.tables, "ts", np.frombuffer(b"".join(struct.pack("<d", v) for v in ts), np.uint64).copy())
        for r, v in zip(recs, ts):
            r.ts = v
    if meta is not None:
        assert len(meta) == n
        m = _column(batch.tables, "meta", np.uint32)
        new = np.array([(0xFF if f is None else f) << 8 | (0xFF if s is None else s) << 16 for f, s in meta], np.uint32)
        m[:n] = (m[:n] & np.uint32(0xFF0000FF)) | new
        _store(batch.tables, "meta", m)
        for r, (f, s) in zip(recs, meta):
            r.facility, r.severity = f, s
    if values is not None:
        val = _column(batch.tables, "ent_val", np.uint64)
        kinds = [t for t in batch.cycle if t != T_SDID]
        assert batch.cycle[:1] != [T_SDID], "typed values are patched into LTSV / GELF rows"
        for ty, vals in values.items():
            cols = [c for c, t in enumerate(kinds) if t == ty]
            assert cols, ty
            k = 0
            for i in range(n):
                pairs = list(recs[i].sd[0].pairs)
                for c in cols:
                    v = vals[k % len(vals)]
                    k += 1
                    bits = struct.unpack("<Q", struct.pack("<d", v))[0] if ty == T_F64 else v & 0xFFFFFFFFFFFFFFFF if ty in (T_I64, T_U64) else int(bool(v))
                    val[idx[i, c]] = bits
                    pairs[c] = (pairs[c][0], SDValue(_KINDS[ty], v))
                recs[i].sd = [dataclasses.replace(recs[i].sd[0], pairs=pairs)]
        _store(batch.tables, "ent_val", val)
    return recs, [to_canonical(r, t) for r, t in zip(recs, batch.ts_now)]


def entries_reserved(batch):
    """the table's ent_used: the entry count that sizes the GELF encoder's ranking scratch"""
    return int(_column(batch.tables, "ent_used", np.uint64)[0])


def patched_values(recs, ty):
    """the values of one pair type in the order patch() consumed its list"""
    return [v.value for r in recs for e in (r.sd or []) for _, v in e.pairs if v.kind == _KINDS[ty]]


def describe(v):
    return v.hex() if isinstance(v, float) else repr(v)


def expected_stream(orc, oenc, canon, merger, extra=None, prepend=None, now_ts=0.0):
    """oracle.encode per row -> (bytes, offsets u64[n + 1], per row None or the error string)"""
    parts, errs = [], []
    for c in canon:
        w = orc.encode(oenc, c, MERGERS[merger], extra=extra, prepend=prepend, now_ts=now_ts)
        errs.append(w if isinstance(w, str) else None)
        parts.append(b"" if isinstance(w, str) else w)
    offs = np.zeros(len(parts) + 1, np.uint64)
    offs[1:] = np.cumsum([len(p) for p in parts])
    return b"".join(parts), offs, errs


def assert_rows(enc, out, off, st, want, woff, errs, label):
    """bytes, offsets and status per row; the message names the first bad row, its value, the GPU bytes and the oracle bytes"""
    assert len(off) == len(woff)
    bad = np.flatnonzero(off != woff)
    i = None
    if len(bad):
        i = max(int(bad[0]) - 1, 0)
    elif out != want:
        a, b = np.frombuffer(out, np.uint8), np.frombuffer(want, np.uint8)
        i = int(np.searchsorted(woff, np.flatnonzero(a != b)[0], side="right") - 1)
    if i is not None:
        raise AssertionError(f"row {i} ({label(i)}):\n  gpu    {out[int(off[i]):int(off[i + 1])][:400]!r}\n  oracle {want[int(woff[i]):int(woff[i + 1])][:400]!r}"
                             f"{'' if errs[i] is None else ' = ' + errs[i]}")
    for i in np.flatnonzero((st != 0) | np.array([e is not None for e in errs])):
        assert enc.error_string(int(st[i])) == errs[i], f"row {i} ({label(i)}): status {st[i]} = {enc.error_string(int(st[i]))!r}, oracle {errs[i]!r}"


def run_and_check(batch, enc, expected, label, now_ts=0.0, use_async=False):
    """one encode of the patched table against `expected` = expected_stream(...) of the same Records, computed once by the caller;
    use_async: fg_encode_device_async into a 0xA5-filled buffer that must stay 0xA5 behind the last byte"""
    import torch

    want, woff, errs = expected
    if use_async:
        buf = torch.full((len(want) + 64,), 0xA5, dtype=torch.uint8, device=batch.d_bytes.device)
        d_off, d_st = enc.encode_device_async(batch.dec, batch.d_bytes, batch.d_offsets, batch.n, batch.tables, buf, now_ts=now_ts)
        torch.cuda.synchronize()
        b = buf.cpu().numpy()
        out = b[:len(want)].tobytes()
        assert (b[len(want):] == 0xA5).all(), "bytes behind the stream were written"
    else:
        d_out, d_off, d_st = enc.encode_device(batch.dec, batch.d_bytes, batch.d_offsets, batch.n, batch.tables, now_ts=now_ts, want_status=True)
        torch.cuda.synchronize()
        out = d_out.cpu().numpy().tobytes()
    assert_rows(enc, out, d_off.cpu().numpy().astype(np.uint64), d_st.cpu().numpy(), want, woff, errs, label)
    return errs
