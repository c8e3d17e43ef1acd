"""GPU: the Cap'n Proto INPUT decoder (FG_CAPNP, k_capnp) through the C ABI -- fg_decode_batch_device and fg_decode_batch --
against the Python model of the reference's reader (tests/capnp_read_model.py), and the ROUND TRIP decode text -> FG_ENC_CAPNP ->
decode FG_CAPNP for every text decoder's corpus; FG_CAPNP tables through the six encoders and the mergers (the oracle's fgo_encode /
capnp_wire.serialize fed with the model's Records) and through fg_transcode_batch."""
import ctypes as C
import math
import struct

import numpy as np
import pytest

import capnp_read_model as M
import capnp_wire as W
from flowgger_amd import _lib as L
from flowgger_amd import synth
from flowgger_amd.record import DecodeError, parse_canonical
from flowgger_amd.tables import DeviceTables, HostTables
from gpu_util import device_path
from test_capnp_in_cpu import ALL_KINDS, ROOT, far_ptr, f64, fuzz_corpus, list_ptr, message, pair_list, same, simple, struct_ptr, text_words, words
from test_gpu_capnp import CORPORA, EXTRA, NOW, decoder, orc  # noqa: F401  (orc: the fixture)

pytestmark = pytest.mark.gpu


def records(tab: HostTables, data, offsets):
    blob, offs = tab.serialize(L.FG_CAPNP, data, offsets)
    raw = blob.tobytes()
    return [parse_canonical(raw[int(offs[i]):int(offs[i + 1])]) for i in range(len(offsets) - 1)]


def gpu_decode(msgs, ent_cap=None, dec=None, allow_overflow=False):
    from flowgger_amd import CapnpDecoder
    from test_capnp_in_cpu import pack_words as pack_messages
    dec = dec or CapnpDecoder()
    data, offsets = pack_messages(msgs)
    tables, _, _ = device_path(dec, data, offsets, ent_cap=ent_cap)
    tab = tables.to_host(allow_overflow=allow_overflow)
    return records(tab, data, offsets), tab, data, offsets


def assert_model(msgs, got):
    for i, m in enumerate(msgs):
        want = M.handle_message(m, max_pairs=1 << 16)
        assert want[0] != "big"
        assert same(got[i], want), (i, m.hex()[:600], got[i], want)


def hand_built():
    import json
    v = bytes(json.loads((ROOT / "tests/golden/capnp_splitter_vector.json").read_text())["message"])
    mk, payload = pair_list(ALL_KINDS)
    mk3, payload3 = pair_list(ALL_KINDS, 3, 3)
    mk1, payload1 = pair_list(ALL_KINDS, 1, 1)
    root = words(struct_ptr(0, 2, 9), f64(3.0), 0x0105)
    seg1_text = words(list_ptr(0, 2, 4)) + text_words(b"far")
    big = W.serialize(W.Record(ts=9.0, hostname="h", full_msg="x" * 69_990 + "é" * 5, sd=[W.StructuredData("id", [("k", W.SDValue("U64", 7))])]))
    return [v, simple(host=None), message(words(0)), simple(dw=1, pw=3), simple(dw=3, pw=12), simple(ts=float("nan")), simple(ts=0.0),
            simple(ts=-1.0), simple(ts=5e-324), simple(d1=31 | 7 << 8), simple(d1=32 | 8 << 8), simple(d1=0xFFFF),
            simple(extra_ptrs={7: (mk, payload)}), simple(extra_ptrs={8: (mk, payload)}), simple(extra_ptrs={7: (mk3, payload3), 8: (mk1, payload1)}),
            simple(extra_ptrs={6: (lambda off: list_ptr(off, 2, 3), text_words(b"id")), 7: (mk, payload), 8: (mk, payload)}),
            simple(extra_ptrs={7: (lambda off: list_ptr(off, 0, 3), b"")}), simple(extra_ptrs={7: (lambda off: list_ptr(off, 1, 9), bytes(8))}),
            message(root + words(far_ptr(1, 0), *[0] * 8), seg1_text),
            message(root + words(far_ptr(1, 0, True), *[0] * 8), words(far_ptr(2, 1), list_ptr(0, 2, 4)), words(0) + text_words(b"dbl")),
            message(root + words(far_ptr(1, 2), *[0] * 8), seg1_text), message(root + words(far_ptr(5, 0), *[0] * 8), seg1_text),
            message(words(far_ptr(1, 0)), words(struct_ptr(0, 2, 9), f64(3.0), 0x0105, *[0] * 9)),
            message(root + words(list_ptr(8, 2, 3), *[0] * 8) + b"\xff\xfe\0\0\0\0\0\0"),
            message(root + words(list_ptr(8, 2, 3), *[0] * 8) + b"abc\0\0\0\0\0"),
            struct.pack("<4I", 1, 12, 100, 0) + root + words(far_ptr(1, 0), *[0] * 8) + seg1_text,
            struct.pack("<2I", 0, 5) + root, struct.pack("<2I", 511, 1) + bytes(8 * 300), words(0), big, v]


def test_reference_vector_and_hand_built_cases():
    msgs = hand_built()
    got, tab, *_ = gpu_decode(msgs)
    assert_model(msgs, got)
    r = got[0]
    assert (r.ts, r.hostname, r.facility, r.severity, r.msgid) == (1385053862.3072, "example.org", None, 1, "")
    assert r.sd[0].sd_id == "someid" and [(k, v.value) for k, v in r.sd[0].pairs] == [("_some_info", "foo")]
    assert len(got[-2].full_msg.encode()) == 70_000   # a message longer than any tile: read from global memory
    # no byte is copied or unescaped: no *_ESC flag; the extras carry FG_EF_NAME_VERBATIM
    # (through ent_first / ent_count: the reserved range holds slots no row refers to, include/fg_hip.h)
    fl = np.concatenate([tab.a["ent_flags"][int(f):int(f) + int(c)] for f, c in zip(tab.a["ent_first"][:len(msgs)], tab.a["ent_count"][:len(msgs)])])
    assert not (fl & (L.FG_EF_VAL_ESC | L.FG_EF_NAME_ESC | L.FG_EF_SUFFIX)).any() and (fl & L.FG_EF_NAME_VERBATIM).any()
    assert not ((tab.a["meta"][:len(msgs)] >> 24) & 0xFF).any()


def test_fuzz_slice_equals_the_model():
    msgs = fuzz_corpus(6000, 20261016)
    keep = [m for m in msgs if M.handle_message(m, max_pairs=4096)[0] != "big"]
    assert len(keep) > 5900
    got, *_ = gpu_decode(keep)
    assert_model(keep, got)


@pytest.mark.parametrize("corpus", ["rfc5424", "rfc5424_sd", "gelf", "ltsv", "rfc3164", "rfc5424_long_tail"])
def test_round_trip(orc, corpus):  # noqa: F811
    """decode -> FG_ENC_CAPNP (capnp_extra configured) -> decode as FG_CAPNP == model(first_sd_only(record)): None texts read back as
    Some(""), facility None preserved, only sd[0], the extras verbatim behind the pairs"""
    import torch

    from flowgger_amd import CapnpDecoder, CapnpEncoder
    src, make = CORPORA[corpus]
    lines = make()
    dec = decoder(src)
    data, offsets = synth.pack(lines)
    tables, d_bytes, d_offsets = device_path(dec, data, offsets)
    extra = EXTRA if corpus != "rfc5424" else None
    enc = CapnpEncoder({"output": {"capnp_extra": extra}} if extra else None)
    d_out, d_off, d_st = enc.encode_device(dec, d_bytes, d_offsets, len(lines), tables, now_ts=NOW, want_status=True)
    torch.cuda.synchronize()
    n = len(lines)
    cdec = CapnpDecoder()
    d_in = torch.cat([d_out, torch.zeros(32, dtype=torch.uint8, device=d_out.device)])
    nbytes = int(d_off[-1].item())
    t2 = DeviceTables(n, nbytes // 8 + 1024, d_out.device)
    cdec.decode_device(d_in, d_off, t2)
    torch.cuda.synchronize()
    out, off = d_out.cpu().numpy(), d_off.cpu().numpy().astype(np.uint64)
    got = records(t2.to_host(), out, off)
    # what the text decoder's Records are, by the oracle
    blob, offs = orc.decode_batch(src, data, offsets, synth.LTSV_CONFIG if src == 1 else None)
    items = sorted((extra or {}).items())
    n_ok = 0
    for i in range(n):
        r = parse_canonical(blob[int(offs[i]):int(offs[i + 1])].tobytes(), now=NOW)
        if isinstance(r, DecodeError):
            assert off[i] == off[i + 1] and str(got[i]) == M.ERR_ROOT   # (an empty message: nothing was encoded for the failed line)
            continue
        want = M.handle_message(W.serialize(W.first_sd_only(r), items))
        assert same(got[i], want), (i, lines[i], got[i], want)
        if want[0] == "ok":
            n_ok += 1
            g = got[i]
            assert g.facility == r.facility and g.severity == r.severity and g.msg == (r.msg or "") and g.appname == (r.appname or "")
            assert len(g.sd) == 1 and [k for k, _ in g.sd[0].pairs][len(g.sd[0].pairs) - len(items):] == [k for k, _ in items]
        else:
            assert math.isnan(r.ts) or r.ts <= 0.0
    assert n_ok > 0.9 * n


def test_host_buffers_zero_copy_and_sliced():
    from flowgger_amd import CapnpDecoder
    from test_capnp_in_cpu import pack_words as pack_messages
    base = [m for m in fuzz_corpus(3000, 5) if M.handle_message(m, max_pairs=4096)[0] != "big"] + hand_built()
    msgs = base * 12
    data, offsets = pack_messages(msgs)
    n = len(msgs)
    want = [M.handle_message(m) for m in base]
    dec = CapnpDecoder()
    lib = L.lib()
    pb, po = C.c_void_p(), C.c_void_p()
    L.check(lib.fg_alloc_pinned(data.size + 64, C.byref(pb)), "fg_alloc_pinned")
    L.check(lib.fg_alloc_pinned((n + 1) * 8, C.byref(po)), "fg_alloc_pinned")
    try:
        hb = np.ctypeslib.as_array(C.cast(pb, C.POINTER(C.c_uint8)), (data.size + 64,))
        ho = np.ctypeslib.as_array(C.cast(po, C.POINTER(C.c_uint64)), (n + 1,))
        hb[:data.size] = data
        hb[data.size:] = 0
        ho[:] = offsets
        paths = []
        for no_zc in (False, True):
            dec.set_launch_opts(no_zero_copy=no_zc)
            st = L.fg_tables()
            L.check(lib.fg_decode_batch(dec._ctx, dec.fmt, pb, data.size, po, n, C.byref(st)), "fg_decode_batch")
            paths.append(int(lib.fg_last_host_path(dec._ctx)))
            got = records(HostTables.from_struct(st), data, offsets)
            for i in range(n):
                assert same(got[i], want[i % len(base)]), (no_zc, i, got[i], want[i % len(base)])
        assert paths == [1, 2]   # FG_PATH_DECODE_ZERO_COPY, FG_PATH_DECODE_SLICED
        # offsets that are no multiples of 8
        ho[1] += 4
        st = L.fg_tables()
        assert lib.fg_decode_batch(dec._ctx, dec.fmt, pb, data.size, po, n, C.byref(st)) == L.FG_ERR_ARG
    finally:
        lib.fg_free_pinned(pb)
        lib.fg_free_pinned(po)
    # the Python classes: decode, decode_batch, the splitter over a stream cut anywhere
    from flowgger_amd import CapnpSplitter
    assert same(dec.decode_batch([m[:len(m) & ~7] for m in base[:50]])[7], want[7])
    with pytest.raises(ValueError):
        dec.decode(base[0] + b"x")   # not a whole number of words
    sp = CapnpSplitter(dec)
    stream = b"".join(m[:len(m) & ~7] for m in hand_built()[:20] if M.frame_stream(m)[1] == len(m))
    outs = sp.feed(stream[:1001]) + sp.feed(stream[1001:1002]) + sp.feed(stream[1002:])
    offs, consumed, err = M.frame_stream(stream)
    assert err is None and consumed == len(stream) and len(outs) == len(offs) - 1
    for i, g in enumerate(outs):
        assert same(g, M.handle_message(stream[offs[i]:offs[i + 1]]))


@pytest.mark.parametrize("n", [1, 63, 65, 4096, 1 << 20])
def test_batch_sizes(n):
    base = hand_built()[:29] + [m for m in fuzz_corpus(500, 3) if M.handle_message(m, max_pairs=256)[0] != "big"]
    want = [M.handle_message(m) for m in base]
    msgs = (base * (n // len(base) + 1))[:n]
    from flowgger_amd import CapnpDecoder
    from test_capnp_in_cpu import pack_words as pack_messages
    data, offsets = pack_messages(msgs)
    tables, _, _ = device_path(CapnpDecoder(), data, offsets)
    tab = tables.to_host()
    step = 1 if n <= 4096 else 9973
    for i in list(range(0, n, step)) + [n - 1]:   # (row by row: a million Records are not materialised in Python)
        blob, offs = tab.serialize(L.FG_CAPNP, data, offsets, i, i + 1)
        g = parse_canonical(blob.tobytes())
        assert same(g, want[i % len(base)]), (n, i, g, want[i % len(base)])
    if n > 4096:   # every row's status and entry count, vectorised
        st = np.array([0 if w[0] == "ok" else {M.ERR_TS: 1, M.ERR_HOST: 2, M.ERR_ROOT: 3}[w[1]] for w in want], np.uint32)
        cnt = np.array([0 if w[0] != "ok" or w[1].sd is None else 1 + len(w[1].sd[0].pairs) for w in want], np.uint32)
        idx = np.arange(n) % len(base)
        assert np.array_equal(tab.a["meta"][:n] & 0xFF, st[idx]) and np.array_equal(tab.a["ent_count"][:n], cnt[idx])


def test_entry_overflow_and_retry():
    import torch

    from flowgger_amd import CapnpDecoder
    from test_capnp_in_cpu import pack_words as pack_messages
    mk, payload = pair_list(ALL_KINDS)
    msgs = [simple(extra_ptrs={7: (mk, payload)})] * 3000
    dec = CapnpDecoder()
    data, offsets = pack_messages(msgs)
    tables, d_bytes, d_offsets = device_path(dec, data, offsets, ent_cap=2000)
    used = int(tables.column("ent_used").view(torch.int64)[0].item())
    assert used > 2000
    with pytest.raises(L.FgError):
        tables.to_host()
    tab = tables.to_host(allow_overflow=True)
    st = tab.a["meta"][:3000] & 0xFF
    assert set(np.unique(st)) == {0, L.FG_ST_OVERFLOW}
    t2 = DeviceTables(3000, used + used // 8, d_bytes.device)
    dec.decode_device(d_bytes, d_offsets, t2)
    torch.cuda.synchronize()
    got = records(t2.to_host(), data, offsets)
    want = M.handle_message(msgs[0])
    assert all(same(g, want) for g in got)
    # the host-buffer entry point grows the table by itself
    assert all(same(g, want) for g in dec.decode_batch(msgs))


def test_launch_geometry_sweep_is_bit_identical():
    from flowgger_amd import CapnpDecoder
    from test_capnp_in_cpu import pack_words as pack_messages
    base = hand_built() + [m for m in fuzz_corpus(3000, 9) if M.handle_message(m, max_pairs=256)[0] != "big"]
    msgs = base * 8
    data, offsets = pack_messages(msgs)
    ref = None
    for opts in ({}, {"lines_per_group": 1}, {"lines_per_group": 7}, {"lines_per_group": 32, "tile_cap": 4096}, {"tile_cap": 8192},
                 {"tile_cap": 57344}, {"static_chunks": True}, {"chunk_lines": 64}, {"waves_per_cu": 1}, {"ent_chunk": 1}):
        dec = CapnpDecoder()
        dec.set_launch_opts(**opts)
        tables, *_ = device_path(dec, data, offsets)
        blob, offs = tables.to_host().serialize(L.FG_CAPNP, data, offsets)
        if ref is None:
            ref = (blob.copy(), offs.copy())
            got = records(tables.to_host(), data, offsets)
            assert_model(base, got[:len(base)])
        else:
            assert np.array_equal(offs, ref[1]) and np.array_equal(blob, ref[0]), opts
        assert dec._ctx and L.lib().fg_ticket_ring_check(dec._ctx) == 0


def test_what_is_refused():
    """framing other than FG_FRAME_NONE (a capnp stream is framed on the host): FG_ERR_ARG, nothing launched"""
    import torch

    from flowgger_amd import CapnpDecoder, GelfEncoder, Pipeline
    from test_capnp_in_cpu import pack_words as pack_messages
    dec = CapnpDecoder()
    data, offsets = pack_messages(hand_built()[:5])
    tables, d_bytes, d_offsets = device_path(dec, data, offsets)
    for framing in (L.FG_FRAME_LINE, L.FG_FRAME_NUL):
        with pytest.raises(L.FgError) as e:
            dec.decode_frames_device(d_bytes, d_offsets, 5, tables, framing)
        assert e.value.code == L.FG_ERR_ARG
        with pytest.raises(L.FgError) as e:
            dec.frame_decode_batch(data.tobytes(), framing)
        assert e.value.code == L.FG_ERR_ARG
    with pytest.raises(L.FgError) as e:
        Pipeline(dec, GelfEncoder()).run_stream(data.tobytes(), L.FG_FRAME_LINE)
    assert e.value.code == L.FG_ERR_ARG
    torch.cuda.synchronize()


# ---- FG_CAPNP tables into the encoders ----------------------------------------------------------------------------------------
def canonical_of(rec):
    """the model's Record in the oracle's canonical form"""
    from test_encoder_cpu import canonical
    sd = None if rec.sd is None else [(e.sd_id, [(k, (W.DISCRIMINANT[v.kind], v.value)) for k, v in e.pairs]) for e in rec.sd]
    return canonical(rec.ts, rec.hostname, rec.facility, rec.severity, rec.appname, rec.procid, rec.msgid, rec.msg, rec.full_msg, sd)


def encoder_corpus():
    """messages whose Records exercise the encoders: pairs of every kind, extras with and without '_' -- one named like a fixed GELF
    member ("host"), one that repeats a pair's key --, sd_id Some / "" / None, texts None, an empty full_msg, multi-segment"""
    mk, payload = pair_list(ALL_KINDS)
    ex = [(b"host", 0, 0, b"h2", False), (b"_s", 0, 0, b"again", False), (b"a", 0, 0, b"", False), (b"zz\tq:", 0, 0, b'v"\t\n\\', False),
          (b"sd_id", 0, 0, b"x", False), (b"_b", 1, 0, None, True), (b"a", 0, 0, b"later", False), (b"version", 0, 0, b"9", False)]
    mke, payloade = pair_list(ex)
    sdid = (lambda off: list_ptr(off, 2, 3), text_words(b"id"))
    bad = (lambda off: list_ptr(off, 3, 1), words(0))          # a getter that fails: None
    badl = (lambda off: struct_ptr(off, 0, 0), b"")                # ... for a list: sd None when all three fail
    txt = lambda t: (lambda off: list_ptr(off, 2, len(t) + 1), text_words(t))  # noqa: E731
    out = [simple(extra_ptrs={7: (mk, payload)}), simple(extra_ptrs={8: (mke, payloade)}), simple(extra_ptrs={6: sdid, 7: (mk, payload), 8: (mke, payloade)}),
           simple(extra_ptrs={6: bad, 7: (mk, payload)}), simple(extra_ptrs={6: bad, 7: bad, 8: bad}), simple(extra_ptrs={6: bad, 7: badl, 8: badl}), simple(extra_ptrs={6: bad}),
           simple(host=b"", extra_ptrs={1: txt(b"app"), 2: txt(b"12"), 3: txt(b"mid"), 4: txt(b"the message"), 5: txt(b"full\nmessage \xc3\xa9")}),
           simple(extra_ptrs={1: bad, 2: bad, 3: bad, 4: bad, 5: bad}), simple(extra_ptrs={5: txt(b"")}), simple(d1=3 | 5 << 8, extra_ptrs={4: txt(b"m")}),
           simple(d1=3 | 0xFF << 8), simple(ts=float("nan")), hand_built()[0]]
    r = __import__("random").Random(77)
    from encode_sweep import qualified
    stamps = [t for t in qualified("timestamps") if 0 < t < math.inf]  # (this route rejects NaN and ts <= 0)
    for _ in range(300):
        items = [(r.choice([b"k%d" % r.randrange(6), b"_k%d" % r.randrange(6), b"shared_prefix_%d" % r.randrange(4), b"\xc3\xa9"]), r.randrange(7), r.getrandbits(64),
                  r.choice([b"v", b"", b'q"\\', b"\xe2\x82\xac"]), r.random() < 0.5) for _ in range(r.choice([0, 1, 3, 9, 40]))]
        exs = [(r.choice([b"x%d" % r.randrange(5), b"_k%d" % r.randrange(6), b"host", b"level", b"timestamp"]), 0, 0, b"e%d" % r.randrange(9), False)
               for _ in range(r.choice([0, 0, 1, 4]))]
        ptrs = {7: pair_list(items), 8: pair_list(exs)}
        if r.random() < 0.5:
            ptrs[6] = sdid
        if r.random() < 0.7:
            ptrs[4] = txt(b"msg %d" % r.randrange(99))
        if r.random() < 0.7:
            ptrs[5] = txt(b"full %d" % r.randrange(99))
        out.append(simple(ts=r.choice([1.5, 1438790025.637824, 1e25] + stamps), d1=r.randrange(40) | r.randrange(10) << 8, extra_ptrs=ptrs))
    big = W.serialize(W.Record(ts=9.0, hostname="h", msg="m", full_msg="x" * 9000, sd=[W.StructuredData("id", [("k", W.SDValue("U64", 7))])]), [("e", "v")])
    return out + [big]


@pytest.mark.parametrize("enc_name", ["gelf", "ltsv", "rfc5424", "rfc3164", "passthrough"])
def test_tables_through_the_text_encoders_and_mergers(orc, enc_name):  # noqa: F811
    import torch

    import oracle_binding as OB
    from flowgger_amd import CapnpDecoder, GelfEncoder, LTSVEncoder, PassthroughEncoder, RFC3164Encoder, RFC5424Encoder
    from test_capnp_in_cpu import pack_words as pack_messages
    cls, oenc, key = {"gelf": (GelfEncoder, OB.ENC_GELF, "gelf_extra"), "ltsv": (LTSVEncoder, OB.ENC_LTSV, "ltsv_extra"),
                      "rfc5424": (RFC5424Encoder, OB.ENC_RFC5424, None), "rfc3164": (RFC3164Encoder, OB.ENC_RFC3164, None),
                      "passthrough": (PassthroughEncoder, OB.ENC_PASSTHROUGH, None)}[enc_name]
    msgs = encoder_corpus()
    models = [M.handle_message(m) for m in msgs]
    dec = CapnpDecoder()
    data, offsets = pack_messages(msgs)
    tables, d_bytes, d_offsets = device_path(dec, data, offsets)
    for merger, mname in enumerate([None, "line", "nul", "syslen"]):
        extra = {"_k1": "shadow", "host": "h3", "a": "", "q": 'v"'} if key and merger in (0, 3) else None
        prepend = "2026-09-23T10:11Z " if enc_name in ("rfc3164", "passthrough") and merger == 1 else None
        enc = cls({"output": {key: extra}} if extra else None, merger=mname, prepend=prepend)
        d_out, d_off, d_st = enc.encode_device(dec, d_bytes, d_offsets, len(msgs), tables, now_ts=NOW, want_status=True)
        torch.cuda.synchronize()
        out, off, st = d_out.cpu().numpy().tobytes(), d_off.cpu().numpy(), d_st.cpu().numpy()
        n_ok = 0
        for i, w in enumerate(models):
            got = out[int(off[i]):int(off[i + 1])]
            if w[0] != "ok":
                assert got == b"" and st[i] == 1, (i, got)
                continue
            want = orc.encode(oenc, canonical_of(w[1]), merger, extra=extra, prepend=prepend, now_ts=NOW)
            if isinstance(want, str):
                assert got == b"" and L.lib().fg_encode_error_string(int(st[i])).decode() == want, (i, want, st[i])
            else:
                n_ok += 1
                assert got == want and st[i] == 0, (enc_name, mname, i, w[1], got, want)
        # (the RFC5424 / RFC3164 encoders need facility AND severity: about 0.8 x 0.8 of the 300 random Records have both; every
        #  encoder must have encoded a good part of the corpus, or the comparison above shows nothing)
        assert n_ok > 100


def test_tables_through_the_capnp_encoder(orc):  # noqa: F811
    import torch

    from flowgger_amd import CapnpDecoder, CapnpEncoder
    from test_capnp_in_cpu import pack_words as pack_messages
    msgs = encoder_corpus()
    models = [M.handle_message(m) for m in msgs]
    dec = CapnpDecoder()
    data, offsets = pack_messages(msgs)
    tables, d_bytes, d_offsets = device_path(dec, data, offsets)
    for merger, extra in ((0, None), (0, EXTRA), (1, EXTRA), (3, None)):
        enc = CapnpEncoder({"output": {"capnp_extra": extra}} if extra else None, merger=[None, "line", "nul", "syslen"][merger])
        d_out, d_off = enc.encode_device(dec, d_bytes, d_offsets, len(msgs), tables, now_ts=NOW)
        torch.cuda.synchronize()
        out, off = d_out.cpu().numpy().tobytes(), d_off.cpu().numpy()
        for i, w in enumerate(models):
            got = out[int(off[i]):int(off[i + 1])]
            want = b"" if w[0] != "ok" else W.frame(W.serialize(w[1], sorted((extra or {}).items())), merger)
            assert got == want, (merger, i, w, got[:300], want[:300])


def test_transcode_batch_capnp_to_gelf(orc):  # noqa: F811
    """the relay's loop (capnp_splitter.rs:47-60) as ONE fg_transcode_batch: one piece and sliced"""
    import oracle_binding as OB
    from flowgger_amd import CapnpDecoder, GelfEncoder, Pipeline
    from test_capnp_in_cpu import pack_words as pack_messages
    base = encoder_corpus()
    models = [M.handle_message(m) for m in base]
    extra = {"_k1": "shadow", "host": "h3"}
    want = [b"" if w[0] != "ok" else orc.encode(OB.ENC_GELF, canonical_of(w[1]), OB.MERGE_LINE, extra=extra, now_ts=NOW) for w in models]
    for reps, one_piece in ((1, False), (90, False), (90, True)):
        msgs = base * reps
        data, offsets = pack_messages(msgs)
        assert reps == 1 or data.size >= 16 << 20
        dec = CapnpDecoder()
        dec.set_launch_opts(transcode_one_piece=one_piece)
        res = Pipeline(dec, GelfEncoder({"output": {"gelf_extra": extra}}, merger="line")).run_packed(data, offsets, now_ts=NOW)
        assert res.n == len(msgs)
        for i in range(len(msgs)):
            w = models[i % len(base)]
            assert res.message(i) == want[i % len(base)], (reps, i, w)
            assert int(res.dec_status[i]) == (0 if w[0] == "ok" else {M.ERR_TS: 1, M.ERR_HOST: 2, M.ERR_ROOT: 3}[w[1]])
    # the splitter form: the stream cut anywhere, a bad table behind good messages
    from flowgger_amd import CapnpStreamError, CapnpTranscodingSplitter
    whole = [m for m in base if len(m) % 8 == 0 and M.frame_stream(m)[1] == len(m)]
    stream = b"".join(whole) + struct.pack("<2I", 511, 0)
    sp = CapnpTranscodingSplitter(GelfEncoder({"output": {"gelf_extra": extra}}, merger="line"), now_ts=NOW)
    got = b"".join(sp.feed(stream[a:b]).out.tobytes() for a, b in ((0, 777), (777, 778), (778, len(stream))))
    assert got == b"".join(want[base.index(m)] for m in whole)
    with pytest.raises(CapnpStreamError):
        sp.feed(b"")
    # offsets that are no multiples of 8
    data, offsets = pack_messages(base)
    offsets = offsets.copy()
    offsets[1] += 4
    with pytest.raises(L.FgError) as e:
        Pipeline(CapnpDecoder(), GelfEncoder()).run_packed(data, offsets)
    assert e.value.code == L.FG_ERR_ARG
