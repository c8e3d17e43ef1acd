"""GPU: the Cap'n Proto encoder (FG_ENC_CAPNP, output.format = "capnp") through the C ABI -- fg_encode_device,
fg_encode_device_async and fg_transcode_batch -- against the oracle's decoded Records serialised by the clean-room wire model
(tests/capnp_wire.py, which reproduces encoder/capnp_encoder.rs's own vectors)."""
import numpy as np
import pytest

import capnp_wire as W
from flowgger_amd import synth
from flowgger_amd.record import DecodeError, parse_canonical
from gpu_util import device_path

pytestmark = pytest.mark.gpu
RFC5424, LTSV, GELF, RFC3164 = 0, 1, 2, 3
NOW = 1438859724.638
EXTRA = {"x-header1": "header1 value", "a": "", "zz": 'q"\t'}


def decoder(src):
    from flowgger_amd import GelfDecoder, LTSVDecoder, RFC3164Decoder, RFC5424Decoder
    return {RFC5424: lambda: RFC5424Decoder(), LTSV: lambda: LTSVDecoder(synth.LTSV_CONFIG), GELF: lambda: GelfDecoder(),
            RFC3164: lambda: RFC3164Decoder({"rfc3164": {"current_year": 2026}})}[src]()


@pytest.fixture(scope="module")
def orc():
    import oracle_binding
    from flowgger_amd import tzdb
    o = oracle_binding.Oracle()
    o.set_rfc3164(2026, tzdb.default_table())
    return o


CORPORA = {
    "rfc5424": (RFC5424, lambda: synth.rfc5424_lines(6000, cfg=2)),
    "rfc5424_sd": (RFC5424, lambda: synth.rfc5424_lines(6000, cfg=4, sd=True)),
    "gelf": (GELF, lambda: synth.gelf_lines(4000)),
    "ltsv": (LTSV, lambda: synth.ltsv_lines(4000)),
    "rfc3164": (RFC3164, lambda: synth.rfc3164_lines(4000)),
    "rfc5424_long_tail": (RFC5424, lambda: synth.rfc5424_lines(3000, cfg=5, sd=True, long_tail=True)),
    "ltsv_long_tail": (LTSV, lambda: synth.ltsv_lines(3000, long_tail=True)),
}


def expected(orc, src, lines, extra=None, now_ts=NOW):
    """per line: the message (b"" for a failed decode) and the encode status"""
    data, offsets = synth.pack(lines)
    blob, offs = orc.decode_batch(src, data, offsets, synth.LTSV_CONFIG if src == LTSV else None)
    items = sorted((extra or {}).items())
    msgs, st = [], []
    for i in range(len(lines)):
        r = parse_canonical(blob[int(offs[i]):int(offs[i + 1])].tobytes(), now=now_ts)
        failed = isinstance(r, DecodeError)
        msgs.append(b"" if failed else W.serialize(r, items))
        st.append(1 if failed else 0)
    return msgs, np.array(st, np.uint8)


def framed(msgs, st, merger):
    parts = [W.frame(m, merger) if s == 0 else b"" for m, s in zip(msgs, st)]
    offs = np.zeros(len(parts) + 1, np.uint64)
    offs[1:] = np.cumsum([len(p) for p in parts])
    return b"".join(parts), offs


def first_bad(out, off, want, woff):
    bad = np.flatnonzero(off != woff)
    i = max(int(bad[0]) - 1, 0) if len(bad) else int(np.searchsorted(woff, np.flatnonzero(
        np.frombuffer(out, np.uint8) != np.frombuffer(want, np.uint8))[0], side="right") - 1)
    return f"line {i}: gpu {out[int(off[i]):int(off[i + 1])][:200]!r}\n want {want[int(woff[i]):int(woff[i + 1])][:200]!r}"


@pytest.mark.parametrize("corpus", list(CORPORA))
def test_encode_device_matches_the_model(orc, corpus):
    import torch

    from flowgger_amd import CapnpEncoder
    src, make = CORPORA[corpus]
    lines = make()
    dec = decoder(src)
    data, offsets = synth.pack(lines)
    tables, d_bytes, d_offsets = device_path(dec, data, offsets)
    extra = EXTRA if corpus in ("rfc5424_sd", "ltsv_long_tail", "gelf") else None
    msgs, st_want = expected(orc, src, lines, extra)
    assert 0 < st_want.sum() < 0.05 * len(lines)  # the corpus's malformed lines are there
    if "long_tail" in corpus:  # rows beyond the first segment occur
        assert any(m and int.from_bytes(m[:4], "little") > 0 for m in msgs)
    mergers = [0, 1, 2, 3] if corpus in ("rfc5424", "rfc5424_long_tail") else [{"gelf": 2, "ltsv": 1, "rfc3164": 3}.get(corpus, 0)]
    for merger in mergers:
        enc = CapnpEncoder({"output": {"capnp_extra": extra}} if extra else None, merger=[None, "line", "nul", "syslen"][merger])
        d_out, d_off, d_st = enc.encode_device(dec, d_bytes, d_offsets, len(lines), tables, now_ts=NOW, want_status=True)
        torch.cuda.synchronize()
        out, off, st = d_out.cpu().numpy().tobytes(), d_off.cpu().numpy().astype(np.uint64), d_st.cpu().numpy()
        want, woff = framed(msgs, st_want, merger)
        assert np.array_equal(st, st_want), "encode status"
        assert np.array_equal(off, woff) and out == want, first_bad(out, off, want, woff)
        # the asynchronous form: the same bytes
        buf = torch.full((len(want) + 64,), 0xA5, dtype=torch.uint8, device=d_bytes.device)
        a_off, a_st = enc.encode_device_async(dec, d_bytes, d_offsets, len(lines), tables, buf, now_ts=NOW)
        torch.cuda.synchronize()
        assert np.array_equal(a_off.cpu().numpy().astype(np.uint64), woff) and np.array_equal(a_st.cpu().numpy(), st_want)
        b = buf.cpu().numpy()
        assert b[:len(want)].tobytes() == want and (b[len(want):] == 0xA5).all()


def test_gelf_rows_without_timestamp_take_now_ts(orc):
    import torch

    from flowgger_amd import CapnpEncoder
    lines = [b'{"version":"1.1","host":"h","short_message":"no timestamp","_k":"v"}', b'{"host":"h2","short_message":"x","timestamp":12.5}']
    dec = decoder(GELF)
    data, offsets = synth.pack(lines)
    tables, d_bytes, d_offsets = device_path(dec, data, offsets)
    d_out, d_off = CapnpEncoder().encode_device(dec, d_bytes, d_offsets, 2, tables, now_ts=777.25)
    torch.cuda.synchronize()
    out, off = d_out.cpu().numpy().tobytes(), d_off.cpu().numpy()
    assert W.parse(out[:int(off[1])])[0].ts == 777.25 and W.parse(out[int(off[1]):])[0].ts == 12.5
    msgs, st = expected(orc, GELF, lines, now_ts=777.25)
    assert out == b"".join(msgs)


@pytest.mark.parametrize("n", [1, 63, 65, 70_000])
def test_batch_sizes(orc, n):
    import torch

    from flowgger_amd import CapnpEncoder
    lines = (synth.rfc5424_lines(3000, cfg=2) + synth.rfc5424_lines(3000, cfg=4, sd=True))
    lines = (lines * (n // len(lines) + 1))[:n]
    dec = decoder(RFC5424)
    data, offsets = synth.pack(lines)
    tables, d_bytes, d_offsets = device_path(dec, data, offsets)
    msgs, st = expected(orc, RFC5424, lines)
    d_out, d_off, d_st = CapnpEncoder(merger="syslen").encode_device(dec, d_bytes, d_offsets, n, tables, now_ts=NOW, want_status=True)
    torch.cuda.synchronize()
    want, woff = framed(msgs, st, 3)
    assert np.array_equal(d_off.cpu().numpy().astype(np.uint64), woff) and d_out.cpu().numpy().tobytes() == want
    assert np.array_equal(d_st.cpu().numpy(), st)


def test_groups_wider_than_the_tile_and_a_million_lines(orc):
    """a 64-line group of 6-9 KiB lines exceeds the LDS tile (the GlobalReader path); 1 M lines = a tile replicated"""
    import torch

    from flowgger_amd import CapnpEncoder
    long_lines = [ln for ln in synth.rfc5424_lines(4000, cfg=5, sd=True, long_tail=True) if len(ln) > 6000][:200]
    assert len(long_lines) >= 64
    tile = synth.rfc5424_lines(4000, cfg=2) + long_lines + synth.rfc5424_lines(2000, cfg=4, sd=True)
    dec = decoder(RFC5424)
    data, offsets = synth.pack(tile)
    msgs, st = expected(orc, RFC5424, tile)
    want, woff = framed(msgs, st, 1)
    reps = 1_000_000 // len(tile) + 1
    tables, d_bytes, d_offsets = device_path(dec, data, offsets, reps=reps)
    n = len(tile) * reps
    d_out, d_off = CapnpEncoder(merger="line").encode_device(dec, d_bytes, d_offsets, n, tables, now_ts=NOW)
    torch.cuda.synchronize()
    off = d_off.cpu().numpy().astype(np.uint64)
    out = d_out.cpu().numpy()
    per = int(woff[-1])
    assert int(off[-1]) == per * reps
    assert np.array_equal(off[:len(tile) + 1], woff)
    for k in (0, 1, reps // 2, reps - 1):
        assert np.array_equal(off[k * len(tile):(k + 1) * len(tile) + 1] - np.uint64(k * per), woff)
        assert out[k * per:(k + 1) * per].tobytes() == want


def test_out_cap_too_small_writes_nothing(orc):
    import torch

    from flowgger_amd import CapnpEncoder
    from flowgger_amd import _lib as L
    import ctypes as C
    lines = synth.rfc5424_lines(500, cfg=2)
    dec = decoder(RFC5424)
    data, offsets = synth.pack(lines)
    tables, d_bytes, d_offsets = device_path(dec, data, offsets)
    enc = CapnpEncoder()
    cfg, _keep = enc._cfg_struct(NOW)
    out = torch.full((1000,), 0x5A, dtype=torch.uint8, device=d_bytes.device)
    d_off = torch.empty(len(lines) + 1, dtype=torch.int64, device=d_bytes.device)
    total = C.c_uint64()
    rc = L.lib().fg_encode_device(dec._ctx, dec.fmt, C.byref(cfg), d_bytes.data_ptr(), d_bytes.numel(), d_offsets.data_ptr(), len(lines),
                                  C.byref(tables.struct), out.data_ptr(), out.numel(), d_off.data_ptr(), None, C.byref(total),
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == L.FG_ERR_ENT_OVERFLOW and total.value > 1000
    assert (out.cpu().numpy() == 0x5A).all()


def test_transcode_batch_packed_and_streams(orc):
    from flowgger_amd import CapnpEncoder, Pipeline
    from flowgger_amd import _lib as L
    dec = decoder(RFC5424)
    pipe = Pipeline(dec, CapnpEncoder({"output": {"capnp_extra": EXTRA}}, merger="nul"))
    # packed lines: small (one piece) and > 16 MiB (the sliced host path, its output size estimated from the first slice)
    small = synth.rfc5424_lines(3000, cfg=2) + synth.rfc5424_lines(3000, cfg=4, sd=True)
    msgs, st = expected(orc, RFC5424, small, EXTRA)
    want, woff = framed(msgs, st, 2)
    for reps in (1, 12):
        lines = small * reps
        data, offsets = synth.pack(lines)
        r = pipe.run_packed(data, offsets, now_ts=NOW)
        assert r.n == len(lines) and np.array_equal(np.minimum(r.enc_status, 2), np.tile(st, reps))
        assert r.out.tobytes() == want * reps
        assert int(r.out_offsets[-1]) == len(want) * reps
    # raw "\n" and NUL streams over several chunks, the unfinished tail carried over
    lines = synth.rfc5424_lines(20_000, cfg=2)
    msgs, st = expected(orc, RFC5424, lines, EXTRA)
    want = b"".join(W.frame(m, 2) for m, s in zip(msgs, st) if s == 0)
    for sep, framing in ((b"\n", L.FG_FRAME_LINE), (b"\0", L.FG_FRAME_NUL)):
        raw = b"".join(ln + sep for ln in lines)
        rng = np.random.default_rng(3)
        out, pos, carry, nf = [], 0, b"", 0
        while True:
            step = int(rng.integers(1, 700_000))
            chunk = carry + raw[pos:pos + step]
            pos += step
            final = pos >= len(raw)
            r = pipe.run_stream(chunk, framing, final=final, now_ts=NOW)
            out.append(r.out.tobytes())
            nf += r.n
            carry = chunk[r.consumed:]
            if final:
                break
        assert nf == len(lines) and b"".join(out) == want
