"""GPU: the one-walk UDP unpacker (fg_udp_unpack_once_device: k_udp_stage, k_udp_write_spilled, k_udp_pack of fg_udp.hip) against the
two-walk one and the model of tests/udp_model.py -- exact on offsets, bytes, drop flags and status, with staged, spilled and bare rows
sharing waves -- and fg_udp_transcode_batch / Pipeline.run_datagrams end to end against model -> oracle decode -> oracle encode +
merger.  Every case first checks ON THE MODEL that it holds what it is there for."""
from __future__ import annotations

import ctypes as C
import gzip
import zlib

import numpy as np
import pytest

import oracle_binding as OB
import test_gpu_udp as TU
import udp_model as um
from flowgger_amd import CapnpEncoder, GelfDecoder, GelfEncoder, Pipeline, UdpUnpacker, synth
from flowgger_amd import _lib as L
from flowgger_amd.record import DecodeError, parse_canonical
from test_gpu_transcode_multi import NOW, expected_stream
from test_inflate_once_cpu import policy_w

pytestmark = pytest.mark.gpu
RFC5424, LTSV, GELF, RFC3164 = 0, 1, 2, 3
CAP = TU.CAP


@pytest.fixture(scope="module")
def dec():
    return GelfDecoder()


@pytest.fixture(scope="module")
def orc(oracle):
    return oracle


def spills(grams, cap):
    """from the model's sizes and the policy alone: which datagrams outgrow their stage"""
    return [um.gate(d) != um.RAW and len(s) > policy_w(d, cap) for d, s in zip(grams, um.expect(grams, cap)[2])]


def unpack_once(dec, grams, cap, out_cap=None):
    import torch

    dev = torch.device("cuda", dec.device)
    blob, offs = um.pack(grams)
    u = UdpUnpacker(dec, cap)
    d_out, d_off, d_drop, d_st = u.unpack_once(TU.to_dev(blob, dev), torch.from_numpy(offs.astype(np.int64)).to(dev), out_cap=out_cap)
    torch.cuda.synchronize(dev)
    return (d_off.cpu().numpy().astype(np.uint64), d_out.cpu().numpy(), d_drop.cpu().numpy(), d_st.cpu().numpy()), u.last_spilled()


def both(dec, grams, cap, what):
    """the one-walk unpack against the model, against the two-walk unpack, and its spilled count against the policy"""
    (offs, packed, drop, st), spilled = unpack_once(dec, grams, cap)
    um.check_batch(grams, cap or um.DEFAULT_MAX, offs, packed, drop, st, what)
    o2, p2, d2, s2 = TU.unpack(dec, grams, cap)
    assert np.array_equal(offs, o2) and np.array_equal(packed, p2) and np.array_equal(drop, d2) and np.array_equal(st, s2), what
    assert spilled == sum(spills(grams, cap or um.DEFAULT_MAX)), what
    return spilled


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_mixed_batch(dec, n):
    mixed = [d for _, d in um.case_list(CAP)] + um.truncations()
    rng = np.random.default_rng(n)
    pick = [mixed[1]] if n == 1 else [mixed[k % len(mixed)] for k in rng.permutation(max(n, len(mixed)))[:n]]
    both(dec, pick, CAP, f"batch of {n}")


def test_whole_case_list_at_the_default_cap(dec):
    assert both(dec, [d for _, d in um.case_list()], None, "case list") >= 3


@pytest.mark.parametrize("cap", um.HAND_CAPS)
def test_hand_streams_in_every_lane(dec, cap):
    both(dec, TU.rotations([d for _, d, _ in um.hand_streams(cap)]), cap, f"hand-built streams, cap {cap}")


def run_of_size(size):
    """a zlib stream of b'ab' * m (+ one byte when size is odd), level 6, that inflates to `size` bytes"""
    return zlib.compress((b"ab" * (size // 2 + 1))[:size], 6)


def test_spilled_staged_and_bare_rows_share_waves(dec):
    cap = 30_000
    edge = []
    for m in (40, 400, 3000):  # a few compressed lengths: w is piecewise constant in the payload's size, so the search ends at once
        d = zlib.compress(b"ab" * m, 6)
        w = policy_w(d, cap)
        for size in (w - 1, w, w + 1):
            e = run_of_size(size)
            for _ in range(8):  # (the stream's length, and with it w, may move with the size: follow it)
                e = run_of_size(policy_w(e, cap) + size - w)
            assert len(um.model(e, cap)[1]) - policy_w(e, cap) == size - w, (m, size - w)
            edge.append(e)
    zeros = zlib.compress(bytes(20_000))
    bad_fit = bytearray(zlib.compress(um.JSON_LINE))
    bad_fit[-1] ^= 1
    bad_spill = bytearray(gzip.compress(b"z" * 9000, mtime=0))
    bad_spill[-6] ^= 1
    exact = zlib.compress(b"q" * 301, 0)
    special = edge + [zeros, bytes(bad_fit), bytes(bad_spill)]
    bare = [b"<%d>short bare record %d" % (k % 190, k) for k in range(200)]
    grams = []
    for k, b in enumerate(bare):  # scattered: every wave of the batch holds bare, staged and spilled rows
        grams.append(b)
        grams.append(special[k % len(special)])
    sp = spills(grams, cap)
    st = um.expect(grams, cap)[0]
    for w0 in range(0, len(grams), 64):
        kinds = {("bare" if um.gate(d) == um.RAW else "spilled" if s else "staged") for d, s in zip(grams[w0:w0 + 64], sp[w0:w0 + 64])}
        assert kinds == {"bare", "spilled", "staged"}, w0
    assert um.model(bytes(bad_fit), cap)[0] == um.BAD_ZLIB and not spills([bytes(bad_fit)], cap)[0] and len(um.model(bytes(bad_fit), cap)[1]) > 300
    assert um.model(bytes(bad_spill), cap)[0] == um.BAD_GZIP and spills([bytes(bad_spill)], cap)[0] and len(um.model(bytes(bad_spill), cap)[1]) == 9000
    assert um.model(zeros, cap)[0] == um.ZLIB and spills([zeros], cap)[0]
    assert both(dec, grams, cap, "spill batch") == sum(sp) > 50
    # the TOO_LARGE row of exactly max_inflated + 1 bytes, with a small cap: it keeps its bytes, staged
    small = [exact, b"bare", zlib.compress(b"q" * 300, 0), zlib.compress(b"q" * 302, 0), zeros] * 13
    assert um.model(exact, 300) == (um.TOO_LARGE, b"q" * 301, False) and policy_w(exact, 300) == 301
    both(dec, small, 300, "exactly one byte too many")


def test_utf8_edges_of_staged_payloads(dec):
    """k_udp_pack's copy_check from a stage slot: a cut-off sequence at the payload's last byte, an offence at bytes 15, 16 and 17 of the
    slot, the payload's length around the 16-byte chunks and the 1024-byte wave stride"""
    probes = TU.UTF8_VALID + TU.UTF8_INVALID
    batch = []
    for length in TU.UTF8_LENGTHS:
        for k, p in enumerate(TU.utf8_payloads(length, probes)):
            batch.append(zlib.compress(p, (0, 1, 6)[k % 3]))
            if k % 4 == 0:
                batch.append(b"-" * (k % 16))  # (bare rows between them: the slots start at every residue)
    st, kept, slots = um.expect(batch, CAP)
    staged = np.array([not s and um.gate(d) != um.RAW for d, s in zip(batch, spills(batch, CAP))])
    assert int(staged.sum()) > 1000 and int((st[staged] == um.BAD_UTF8).sum()) > 500 and int(kept[staged].sum()) > 300
    for at in (15, 16, 17):
        assert any(s[at:at + 1] == b"\x80" and x for s, x in zip(slots, staged))
    assert any(x and len(s) > 1 and s[-2:-1] != b"\xc3" and s[-1:] == b"\xc3" for s, x in zip(slots, staged))  # cut off at the last byte
    both(dec, batch, CAP, "UTF-8 edges of staged payloads")


def test_no_sizing_call_and_an_exact_buffer(dec):
    import torch

    grams = ([d for _, d in um.case_list(CAP)] + um.truncations())[:300]
    dev = torch.device("cuda", dec.device)
    blob, offs = um.pack(grams)
    n = len(grams)
    d_bytes, d_offs = TU.to_dev(blob, dev), torch.from_numpy(offs.astype(np.int64)).to(dev)
    d_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_drop, d_st = torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev)
    total = C.c_uint64()
    head = (dec._ctx, d_bytes.data_ptr(), d_bytes.numel(), d_offs.data_ptr(), n, CAP)
    tail = (d_off.data_ptr(), d_drop.data_ptr(), d_st.data_ptr(), C.byref(total), None)
    lib = L.lib()
    assert lib.fg_udp_unpack_once_device(*head, None, 0, *tail) == L.FG_ERR_ARG
    need = sum(len(s) for s in um.expect(grams, CAP)[2])
    d_out = torch.full(((need + 15) // 16 * 16 + 16,), 0xEE, dtype=torch.uint8, device=dev)
    assert lib.fg_udp_unpack_once_device(*head, d_out.data_ptr(), need - 1, *tail) == L.FG_ERR_ENT_OVERFLOW and int(total.value) == need
    torch.cuda.synchronize(dev)
    assert bool((d_out == 0xEE).all()), "an overflowing call wrote payload bytes"
    assert lib.fg_udp_unpack_once_device(*head, d_out.data_ptr(), need, *tail) == L.FG_OK and int(total.value) == need
    torch.cuda.synchronize(dev)
    out = d_out.cpu().numpy()
    um.check_batch(grams, CAP, d_off.cpu().numpy().astype(np.uint64), out, d_drop.cpu().numpy(), d_st.cpu().numpy(), "exact capacity")
    assert bool((out[need:] == 0xEE).all()), "bytes written behind the last payload"


# ---- fg_udp_transcode_batch ---------------------------------------------------------------------------------------------------------
def transcode_case(fmt, seed):
    """about 600 datagrams: raw, zlib and gzip lines of the format, every drop reason, lines that fail to decode, streams that spill"""
    lines = TU.corpus(fmt, 560)
    grams = TU.datagrams_of(lines, seed)
    cases = dict(um.case_list(CAP))
    extra = [cases[k] for k in ("raw_bad_utf8", "zlib_bad_utf8", "gzip_cut_utf8", "zlib_bad_adler", "gz_bad_crc32", "gz_bad_fhcrc", "match_past_cap",
                                "match_past_cap_gz", "gz_isize_cut")]
    extra += [b"this is no log line at all", zlib.compress(b"neither is this"), gzip.compress(b"nor this one here, it is long enough", mtime=0), zlib.compress(b""),
              zlib.compress(b" " * 3000)]
    rng = np.random.default_rng(seed)
    for e in extra * 3:
        grams.insert(int(rng.integers(len(grams))), e)
    return grams


def expected_udp(orc, fmt, cfg, oenc, grams, cap):
    """-> (stream, size per datagram, udp_status, decode failed per datagram, stderr lines)"""
    st, kept, slots = um.expect(grams, cap)
    bodies = [s for s, k in zip(slots, kept) if k]
    stream, sizes, failed = expected_stream(orc, fmt, cfg, oenc, bodies)
    data, offsets = synth.pack(bodies)
    blob, offs = orc.decode_batch(fmt, data, offsets, cfg)
    it = iter(range(len(bodies)))
    size_of, failed_of, err = [], [], []
    for i in range(len(grams)):
        if not kept[i]:
            size_of.append(0)
            failed_of.append(None)
            err.append(um.ERRORS.get(int(st[i])) or L.lib().fg_udp_error_string(int(st[i])).decode())
            continue
        j = next(it)
        size_of.append(sizes[j])
        failed_of.append(failed[j])
        if failed[j] == 1:
            r = parse_canonical(blob[int(offs[j]):int(offs[j + 1])].tobytes(), now=NOW)
            assert isinstance(r, DecodeError)
            err.append(str(r))
        elif failed[j]:
            e = orc.encode(oenc[0], blob[int(offs[j]):int(offs[j + 1])].tobytes(), oenc[1], now_ts=NOW)
            assert isinstance(e, str)
            err.append(e)
    return stream, size_of, st, failed_of, err


ENCODERS = {"gelf_line": (lambda: GelfEncoder(None, merger="line"), (OB.ENC_GELF, OB.MERGE_LINE)), "capnp_syslen": (lambda: CapnpEncoder(None, merger="syslen"), ("capnp", 3))}


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
@pytest.mark.parametrize("enc", ["gelf_line", "capnp_syslen"])
@pytest.mark.parametrize("fmt", [GELF, RFC5424, LTSV, RFC3164], ids=["gelf", "rfc5424_sd", "ltsv", "rfc3164"])
def test_udp_transcode_batch_end_to_end(orc, fmt, enc, pinned):
    d, cfg = TU.make_decoder(fmt, orc)
    make_enc, oenc = ENCODERS[enc]
    grams = transcode_case(fmt, 200 + fmt)
    stream, sizes, st, failed, err = expected_udp(orc, fmt, cfg, oenc, grams, CAP)
    assert set(st.tolist()) == set(range(7)) and sum(1 for f in failed if f == 1) >= 3 and sum(1 for s in sizes if s) > 500 and sum(spills(grams, CAP)) >= 3
    blob, offs = um.pack(grams)
    held = []
    if pinned:
        held = [TU.Pinned(blob.size + 32), TU.Pinned((len(offs) + 2) * 8)]
        pb, po = held[0].array(np.uint8, blob.size + 32), held[1].array(np.uint64, len(offs))
        pb[:blob.size] = blob
        po[:] = offs
        blob, offs = pb[:blob.size], po
    try:
        path_before = L.lib().fg_last_host_path(d._ctx)
        t = Pipeline(d, make_enc()).run_datagrams((blob, offs), max_inflated=CAP, now_ts=NOW)
        assert L.lib().fg_last_host_path(d._ctx) == path_before
        assert L.lib().fg_udp_last_spilled(d._ctx) == sum(spills(grams, CAP))
        n = len(grams)
        assert t.n == n and t.consumed == blob.size and t.frame_offsets is None
        assert np.array_equal(t.udp_status, st)
        assert np.diff(t.out_offsets.astype(np.int64)).tolist() == sizes and int(t.out_offsets[0]) == 0
        assert t.out.tobytes() == stream
        for i in range(n):
            if failed[i] is None:
                assert t.dec_status[i] == L.FG_ST_BAD_UTF8 and t.enc_status[i] == 1, i
            else:
                assert (t.dec_status[i] != 0) == (failed[i] == 1) and (t.enc_status[i] == 0) == (sizes[i] > 0), i
        assert t.stderr_lines() == err
        assert b"".join(t.message(i) for i in range(n) if sizes[i]) == stream
    finally:
        for h in held:
            h.free()
        d.close()


def test_no_kept_datagram_a_batch_of_one_and_a_packed_batch_right_after(orc):
    d = GelfDecoder()
    p = Pipeline(d, GelfEncoder(None, merger="line"))
    try:
        none = [b"\xff", zlib.compress(b"abc")[:-1], gzip.compress(b"abcdefgh", mtime=0)[:-3], b"\xc3"]
        t = p.run_datagrams(none, now_ts=NOW)
        assert t.n == 4 and t.out.size == 0 and t.out_offsets.tolist() == [0] * 5 and t.udp_status.tolist() == um.expect(none)[0].tolist()
        assert t.stderr_lines() == [um.ERRORS[int(s)] for s in um.expect(none)[0]] and t.enc_status.tolist() == [1] * 4
        line = TU.corpus(GELF, 1)[0]
        want = expected_stream(orc, GELF, None, (OB.ENC_GELF, OB.MERGE_LINE), [line])
        for one in (line, zlib.compress(line), gzip.compress(line, mtime=0)):
            t = p.run_datagrams([one], now_ts=NOW)
            assert t.out.tobytes() == want[0] and t.stderr_lines() == [] and len(want[0]) > 20
        assert p.run_datagrams([], now_ts=NOW).n == 0
        # the ctx's buffers are shared with fg_transcode_batch: a packed batch right after, and datagrams after that
        lines = TU.corpus(GELF, 300)
        data, offsets = synth.pack(lines)
        want = expected_stream(orc, GELF, None, (OB.ENC_GELF, OB.MERGE_LINE), lines)
        assert p.run_packed(data, offsets, now_ts=NOW).out.tobytes() == want[0]
        t = p.run_datagrams([zlib.compress(x) if i % 2 else x for i, x in enumerate(lines)], now_ts=NOW)
        assert t.out.tobytes() == want[0]
        assert p.run_packed(data, offsets, now_ts=NOW).out.tobytes() == want[0]
    finally:
        d.close()


def test_capnp_and_bad_arguments_are_rejected():
    from flowgger_amd import CapnpDecoder

    d = CapnpDecoder()
    with pytest.raises(Exception):
        Pipeline(d, GelfEncoder(None, merger="line")).run_datagrams([b"abc"])
    d.close()
