"""GPU tests of the UDP input's body on the device (flowgger_amd/csrc/fg_udp.hip / fg_inflate.hpp; fg_udp_unpack_device,
fg_udp_decode_batch) through the C ABI, against the model of handle_record_maybe_compressed -- the reference's gate, then Python's
zlib (tests/udp_model.py) -- and the oracle decoders on the model's inflated lines.  Exact on verdict and bytes."""
from __future__ import annotations

import ctypes as C
import gzip
import zlib

import numpy as np
import pytest

import udp_model as um
from flowgger_amd import GelfDecoder, LTSVDecoder, RFC3164Decoder, RFC5424Decoder, UdpUnpacker, synth, tzdb
from flowgger_amd import _lib as L
from golden.reference_vectors import RFC3164_CONFIG, RFC3164_YEAR

pytestmark = pytest.mark.gpu
RFC5424, LTSV, GELF, RFC3164 = 0, 1, 2, 3
CAP = 4096  # max_inflated of the mixed batches: the cases at the cap stay small


@pytest.fixture(scope="module")
def dec():
    return GelfDecoder()


@pytest.fixture(scope="module")
def mixed():
    """the CPU suite's case list and every truncation, as one pool"""
    return [d for _, d in um.case_list(CAP)] + um.truncations()


def to_dev(blob, dev):
    import torch

    buf = np.zeros((blob.size + 15) // 16 * 16 + 16, np.uint8)
    buf[:blob.size] = blob
    return torch.from_numpy(buf).to(dev)[:blob.size]


def unpack(dec, datagrams, max_inflated):
    import torch

    dev = torch.device("cuda", dec.device)
    blob, offs = um.pack(datagrams)
    d_out, d_off, d_drop, d_st = UdpUnpacker(dec, max_inflated).unpack(to_dev(blob, dev), torch.from_numpy(offs.astype(np.int64)).to(dev))
    torch.cuda.synchronize(dev)
    return d_off.cpu().numpy().astype(np.uint64), d_out.cpu().numpy(), d_drop.cpu().numpy(), d_st.cpu().numpy()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_mixed_batch_matches_the_model(dec, mixed, n):
    """raw, zlib, gzip, corrupt and too-large datagrams sharing waves"""
    rng = np.random.default_rng(n)
    pick = [mixed[1]] if n == 1 else [mixed[k % len(mixed)] for k in rng.permutation(max(n, len(mixed)))[:n]]
    offs, packed, drop, st = unpack(dec, pick, CAP)
    um.check_batch(pick, CAP, offs, packed, drop, st, f"batch of {n}")


def test_whole_case_list_at_the_default_cap(dec):
    cases = [d for _, d in um.case_list()]
    offs, packed, drop, st = unpack(dec, cases, None)
    um.check_batch(cases, um.DEFAULT_MAX, offs, packed, drop, st, "case list")


def test_sizing_call_exact_capacity_and_overflow(dec, mixed):
    import torch

    dev = torch.device("cuda", dec.device)
    blob, offs = um.pack(mixed)
    n = len(mixed)
    d_bytes, d_offs = to_dev(blob, dev), torch.from_numpy(offs.astype(np.int64)).to(dev)
    d_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_drop, d_st = torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev)
    total = C.c_uint64()
    head = (dec._ctx, d_bytes.data_ptr(), d_bytes.numel(), d_offs.data_ptr(), n, CAP)
    tail = (d_off.data_ptr(), d_drop.data_ptr(), d_st.data_ptr(), C.byref(total), None)
    lib = L.lib()
    assert lib.fg_udp_unpack_device(*head, None, 0, *tail) == L.FG_OK
    _, _, slots = um.expect(mixed, CAP)
    need = int(total.value)
    assert need == sum(len(s) for s in slots)
    d_out = torch.full(((need + 15) // 16 * 16 + 16,), 0xEE, dtype=torch.uint8, device=dev)
    assert lib.fg_udp_unpack_device(*head, d_out.data_ptr(), need - 1, *tail) == L.FG_ERR_ENT_OVERFLOW
    assert int(total.value) == need
    assert bool((d_out == 0xEE).all()), "an overflowing call wrote payload bytes"
    assert lib.fg_udp_unpack_device(*head, d_out.data_ptr(), need, *tail) == L.FG_OK
    assert int(total.value) == need
    torch.cuda.synchronize(dev)
    out = d_out.cpu().numpy()
    um.check_batch(mixed, CAP, d_off.cpu().numpy().astype(np.uint64), out, d_drop.cpu().numpy(), d_st.cpu().numpy(), "exact capacity")
    assert bool((out[need:] == 0xEE).all()), "bytes written behind the last payload"


def test_error_strings():
    lib = L.lib()
    assert lib.fg_udp_error_string(3) == b"Corrupted compressed (zlib) record"
    assert lib.fg_udp_error_string(4) == b"Corrupted compressed (gzip) record"
    assert lib.fg_udp_error_string(5) == b"Invalid UTF-8 input"
    assert [lib.fg_udp_error_string(k) for k in (0, 1, 2)] == [b"", b"", b""]
    assert lib.fg_udp_error_string(6) and lib.fg_udp_error_string(7) is None


def test_mutation_pool_in_one_launch(dec):
    pool = um.mutation_pool()
    offs, packed, drop, st = unpack(dec, pool, None)
    um.check_batch(pool, um.DEFAULT_MAX, offs, packed, drop, st, "mutation pool")


def rotations(cases, filler=b"pad"):
    """the list, filled up to whole waves, 64 times over and shifted by one lane each time: every case sits in every lane once, next
    to 63 other cases"""
    padded = list(cases) + [filler] * (-len(cases) % 64)
    return [padded[(k - j) % len(padded)] for j in range(64) for k in range(len(padded))]


@pytest.mark.parametrize("cap", um.HAND_CAPS)
def test_hand_streams_share_waves(dec, cap):
    """the hand-built streams (tests/deflate_build.py) with 64 different code sets and verdicts per wave, every case in every lane
    (lanes 0 and 63 among them); then a wave whose 64 lanes hold the same dynamic block; then a last wave of one lane"""
    table = um.hand_streams(cap)
    cases = [d for _, d, _ in table]
    same = dict((n, d) for n, d, _ in table)["all_286_and_30_symbols_hlit29_hdist29_z"]
    batch = rotations(cases) + [same] * 64 + [cases[0]]
    assert len(batch) % 64 == 1
    offs, packed, drop, st = unpack(dec, batch, cap)
    um.check_batch(batch, cap, offs, packed, drop, st, f"hand-built streams, cap {cap}")
    want = {d: w for n, d, w in table if n.startswith("cap_") or cap == um.DEFAULT_MAX}
    for d, got in zip(batch[:len(cases)], st):  # (the first rotation is the list itself; the table's verdicts, not only the model's)
        assert d not in want or got == want[d]
    # every case once in a last, partial wave: 63 of them behind whole waves of the others
    for s in range(0, len(cases), 63):
        last = cases[s:s + 63]
        front = cases[s + 63:] + cases[:s]
        batch = front + [b"pad"] * (-len(front) % 64) + last
        assert 0 < len(batch) % 64 == len(last)
        offs, packed, drop, st = unpack(dec, batch, cap)
        um.check_batch(batch, cap, offs, packed, drop, st, f"hand-built streams, cap {cap}, last wave from {s}")
    if cap == um.DEFAULT_MAX:  # whole waves only, and whole waves plus one
        for n in (len(cases) // 64 * 64, len(cases) // 64 * 64 + 1):
            offs, packed, drop, st = unpack(dec, cases[:n], cap)
            um.check_batch(cases[:n], cap, offs, packed, drop, st, f"hand-built streams, n = {n}")


def test_random_code_sets(dec):
    good, flipped = um.random_code_set_pool()
    pool = [d for pair in zip(good, flipped) for d in pair]  # (valid and broken streams side by side in every wave)
    offs, packed, drop, st = unpack(dec, pool, None)
    um.check_batch(pool, um.DEFAULT_MAX, offs, packed, drop, st, "random code sets")
    assert int((st[0::2] <= um.GZIP).sum()) == len(good)


UTF8_VALID = [b"\xc3\xa9", b"\xe2\x9c\x93", b"\xf0\x9f\x98\x80", b"\xe0\xa0\x80", b"\xed\x9f\xbf", b"\xf0\x90\x80\x80", b"\xf4\x8f\xbf\xbf"]
UTF8_INVALID = [b"\xc0\x80", b"\xc1\xbf", b"\xe0\x9f\x80", b"\xed\xa0\x80", b"\xf0\x8f\x80\x80", b"\xf4\x90\x80\x80", b"\xf5\x80\x80\x80", b"\x80",
                b"\xc3A", b"\xe2\x9cA", b"\xf0\x9f\x98A"]
UTF8_LENGTHS = (1, 15, 16, 17, 31, 32, 33, 1023, 1024, 1025, 1040, 2048, 2049)


def utf8_payloads(length, probes):
    """ASCII filler with one probe whose first byte lands at each of the offsets; a probe that does not fit is cut off by the payload's
    end (after 1, 2 or 3 bytes: the offsets len - 3 .. len - 1)"""
    fill = (b"0123456789abcdefghijklmnopqrstuvwxyz" * (length // 36 + 1))[:length]
    offsets = sorted({o for o in (0, 1, 13, 14, 15, 16, 17, 1021, 1022, 1023, 1024, 1025, length - 3, length - 2, length - 1) if 0 <= o < length})
    out = []
    for o in offsets:
        for p in probes:
            out.append((fill[:o] + p + fill[o + len(p):])[:length])
            assert len(out[-1]) == length
    return out


def unpack_exact(dec, datagrams, max_inflated):
    """as unpack(), through the sizing call and then into a buffer of exactly the size it named, filled with 0xEE: nothing behind the
    last slot is written (and check_batch holds every slot against its neighbours)"""
    import torch

    dev = torch.device("cuda", dec.device)
    blob, offs = um.pack(datagrams)
    n = len(datagrams)
    d_bytes, d_offs = to_dev(blob, dev), torch.from_numpy(offs.astype(np.int64)).to(dev)
    d_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_drop, d_st = torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev)
    total = C.c_uint64()
    head = (dec._ctx, d_bytes.data_ptr(), d_bytes.numel(), d_offs.data_ptr(), n, max_inflated)
    tail = (d_off.data_ptr(), d_drop.data_ptr(), d_st.data_ptr(), C.byref(total), None)
    lib = L.lib()
    assert lib.fg_udp_unpack_device(*head, None, 0, *tail) == L.FG_OK
    need = int(total.value)
    d_out = torch.full(((need + 15) // 16 * 16 + 16,), 0xEE, dtype=torch.uint8, device=dev)
    assert d_out.data_ptr() % 16 == 0
    assert lib.fg_udp_unpack_device(*head, d_out.data_ptr(), need, *tail) == L.FG_OK
    torch.cuda.synchronize(dev)
    out = d_out.cpu().numpy()
    assert bool((out[need:] == 0xEE).all()), "bytes written behind the last payload"
    return d_off.cpu().numpy().astype(np.uint64), out, d_drop.cpu().numpy(), d_st.cpu().numpy()


def test_utf8_edges_of_inflated_and_bare_payloads(dec):
    """utf8_bad() on inflated payloads and copy_check() on bare ones, which the CPU build replaces by a bytewise loop: a probe at the
    16-byte chunk edges, at the 1024-byte wave stride and at the payload's end, the payload's length around the same edges, and for
    the bare ones the slot starting at every residue mod 16 (copy_check's unaligned head).  The answer is bytes.decode's."""
    probes = UTF8_VALID + UTF8_INVALID
    batch, slot_at, seen = [], 0, set()

    def put(d, size):  # (every datagram here keeps a slot of its payload's size, dropped for its UTF-8 or not)
        nonlocal slot_at
        batch.append(d)
        slot_at += size

    # three ways: bare, zlib, gzip
    for length in UTF8_LENGTHS:
        for k, p in enumerate(utf8_payloads(length, probes)):
            put(p, length)
            put(zlib.compress(p, (0, 1, 6)[k % 3]), length)
            put(um.gz_member(p, level=(6, 0, 9)[k % 3], name=b"edge" if length < 16 else None), length)  # (24 bytes for the gate)
            assert um.gate(batch[-1]) == um.GZIP and um.gate(batch[-2]) == um.ZLIB and um.gate(batch[-3]) == um.RAW
    # the bare ones again with the slot at every residue: the short lengths whole, the long ones (whose head is filler unless the probe
    # is among the first 17 bytes) with three probes
    few = [UTF8_VALID[2], UTF8_INVALID[3], UTF8_INVALID[7]]
    for h in range(16):
        for length in UTF8_LENGTHS:
            for p in utf8_payloads(length, probes if length <= 33 else few):
                if slot_at % 16 != h:
                    put(b"-" * ((h - slot_at) % 16), (h - slot_at) % 16)
                seen.add((h, length))
                put(p, length)
    assert len(seen) == 16 * len(UTF8_LENGTHS)
    st_model, kept, slots = um.expect(batch, CAP)
    assert int(kept.sum()) > 1000 and int((st_model == um.BAD_UTF8).sum()) > 1000 and not bool((st_model == um.TOO_LARGE).any())
    assert sum(len(s) for s in slots) == slot_at
    offs, packed, drop, st = unpack_exact(dec, batch, CAP)
    um.check_batch(batch, CAP, offs, packed, drop, st, "UTF-8 edges")


def test_hand_built_gelf_streams_end_to_end(oracle):
    """64 GELF lines in hand-built streams over random code sets, one wave of them, through fg_udp_decode_batch: rows against the oracle"""
    d = GelfDecoder()
    rng = np.random.default_rng(1953)
    import deflate_build as db

    lines = corpus(GELF, 64)
    grams = [(db.wrap_zlib if k % 2 else db.wrap_gzip)(db.random_dynamic_stream(rng, l), l) for k, l in enumerate(lines)]
    try:
        blob, offs = um.pack(grams)
        tab, out_lines, line_offs, ust = d.udp_decode_packed(blob, offs)
        st, kept, slots = um.expect(grams)
        assert bool(kept.all()) and np.array_equal(ust, st) and slots == lines
        gblob, goffs = tab.serialize(d.fmt, out_lines, line_offs, cfg=d._cfg)
        mblob, moffs = um.pack(lines)
        oblob, ooffs = oracle.decode_batch(GELF, np.concatenate([mblob, np.zeros(16, np.uint8)]), moffs, config=None)
        for i in range(64):
            assert bytes(out_lines[int(line_offs[i]):int(line_offs[i + 1])]) == lines[i], f"inflated line {i}"
            a, b = gblob[int(goffs[i]):int(goffs[i + 1])].tobytes(), oblob[int(ooffs[i]):int(ooffs[i + 1])].tobytes()
            assert a == b, f"row {i}: {lines[i]!r}\n  gpu    {a!r}\n  oracle {b!r}"
    finally:
        d.close()


def make_decoder(fmt, oracle):
    if fmt == RFC5424:
        return RFC5424Decoder(), None
    if fmt == LTSV:
        return LTSVDecoder(synth.LTSV_CONFIG), synth.LTSV_CONFIG
    if fmt == GELF:
        return GelfDecoder(), None
    oracle.set_rfc3164(RFC3164_YEAR, tzdb.default_table())
    return RFC3164Decoder(RFC3164_CONFIG), None  # (the oracle has the year and the zone table from set_rfc3164)


def corpus(fmt, n):
    lines = {RFC5424: lambda: synth.rfc5424_lines(n, cfg=2, sd=True), LTSV: lambda: synth.ltsv_lines(n), GELF: lambda: synth.gelf_lines(n),
             RFC3164: lambda: synth.rfc3164_lines(n)}[fmt]()
    return [(l if isinstance(l, bytes) else l.encode()).rstrip(b"\n") for l in lines]


def datagrams_of(lines, seed):
    """a third bare, a third zlib, a third gzip; 1 % corrupted"""
    rng = np.random.default_rng(seed)
    out = []
    for i, l in enumerate(lines):
        d = l if i % 3 == 0 else zlib.compress(l, (1, 6, 9)[i % 9 // 3]) if i % 3 == 1 else gzip.compress(l, mtime=0)
        if rng.random() < 0.01 and len(d) > 12:
            d = bytearray(d)
            d[int(rng.integers(8, len(d)))] ^= 1 << int(rng.integers(8))
            d = bytes(d)
        out.append(d)
    return out


class Pinned:
    def __init__(self, nbytes):
        self.p = C.c_void_p()
        L.check(L.lib().fg_alloc_pinned(nbytes, C.byref(self.p)), "fg_alloc_pinned")

    def array(self, dtype, count):
        return np.ctypeslib.as_array(C.cast(self.p, C.POINTER(C.c_uint8)), (count * np.dtype(dtype).itemsize,)).view(dtype)

    def free(self):
        L.lib().fg_free_pinned(self.p)


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
@pytest.mark.parametrize("fmt", [GELF, RFC5424, LTSV, RFC3164], ids=["gelf", "rfc5424_sd", "ltsv", "rfc3164"])
def test_udp_decode_batch_end_to_end(oracle, fmt, pinned):
    d, cfg = make_decoder(fmt, oracle)
    grams = datagrams_of(corpus(fmt, 4000), 100 + fmt)
    blob, offs = um.pack(grams)
    held = []
    if pinned:
        held = [Pinned(blob.size + 32), Pinned((len(offs) + 2) * 8)]
        pb, po = held[0].array(np.uint8, blob.size + 32), held[1].array(np.uint64, len(offs))
        pb[:blob.size] = blob
        po[:] = offs
        blob, offs = pb[:blob.size], po
    try:
        path_before = L.lib().fg_last_host_path(d._ctx)
        tab, lines, line_offs, ust = d.udp_decode_packed(blob, offs)
        assert L.lib().fg_last_host_path(d._ctx) == path_before
        st, kept, slots = um.expect(grams)
        assert np.array_equal(ust, st)
        assert kept.sum() > 3500 and (~kept).sum() > 5
        n = len(grams)
        status = tab.status[:n]
        assert bool((status[~kept] == L.FG_ST_BAD_UTF8).all()), "a dropped datagram was decoded"
        # canonical Record bytes of every kept row against the oracle on the model's inflated line
        gblob, goffs = tab.serialize(d.fmt, lines, line_offs, cfg=d._cfg)
        model_lines = [s if k else b"" for s, k in zip(slots, kept)]
        mblob, moffs = um.pack(model_lines)
        oblob, ooffs = oracle.decode_batch(fmt, np.concatenate([mblob, np.zeros(16, np.uint8)]), moffs, config=cfg)
        for i in np.flatnonzero(kept):
            assert bytes(lines[int(line_offs[i]):int(line_offs[i + 1])]) == slots[i], f"inflated line {i}"
            a, b = gblob[int(goffs[i]):int(goffs[i + 1])].tobytes(), oblob[int(ooffs[i]):int(ooffs[i + 1])].tobytes()
            assert a == b, f"row {i}: {slots[i]!r}\n  gpu    {a!r}\n  oracle {b!r}"
    finally:
        for h in held:
            h.free()
        d.close()


def dense_ltsv_datagrams(n=30, pairs=100):
    """LTSV lines of many short pairs (five bytes each), a third bare, a third zlib, a third gzip: more entries than one per eight
    inflated bytes plus 1024, the entry table fg_udp_decode_batch starts with.  30 datagrams of 100 pairs are the fewest: 3000 entries
    in 15 710 bytes (2987 slots to start with); 29 hold 2900 in 15 186 (2922 slots)"""
    keys = [bytes([a, b]) for a in range(97, 123) for b in range(97, 123)]
    lines = [b"time:%d\thost:h%d\t" % (1_600_000_000 + i, i) + b"\t".join(k + b":%d" % ((i + j) % 10) for j, k in enumerate(keys[i:i + pairs]))
             for i in range(n)]
    grams = [l if i % 3 == 0 else zlib.compress(l, 6) if i % 3 == 1 else gzip.compress(l, mtime=0) for i, l in enumerate(lines)]
    return lines, grams


def test_udp_decode_batch_grows_the_entry_table(oracle):
    """a batch whose entries outnumber the first guess (inflated bytes / 8 + 1024): the decode is repeated with the table the counter
    asked for, and every row and entry is the oracle's"""
    from flowgger_amd.record import Record, parse_canonical

    lines, grams = dense_ltsv_datagrams()
    mblob, moffs = um.pack(lines)
    oblob, ooffs = oracle.decode_batch(LTSV, np.concatenate([mblob, np.zeros(16, np.uint8)]), moffs, config=synth.LTSV_CONFIG)
    recs = [parse_canonical(oblob[int(ooffs[i]):int(ooffs[i + 1])].tobytes()) for i in range(len(lines))]
    assert all(isinstance(r, Record) for r in recs)
    entries = sum(len(sd.pairs) for r in recs for sd in r.sd)
    assert entries > int(mblob.size) // 8 + 1024, (entries, int(mblob.size))
    d = LTSVDecoder(synth.LTSV_CONFIG)
    try:
        blob, offs = um.pack(grams)
        tab, out_lines, line_offs, ust = d.udp_decode_packed(blob, offs)
        st, kept, slots = um.expect(grams)
        assert bool(kept.all()) and np.array_equal(ust, st) and slots == lines
        assert int(tab.a["ent_count"][:len(lines)].sum()) == entries and not bool((tab.status[:len(lines)] == L.FG_ST_OVERFLOW).any())
        gblob, goffs = tab.serialize(d.fmt, out_lines, line_offs, cfg=d._cfg)
        for i in range(len(lines)):
            a, b = gblob[int(goffs[i]):int(goffs[i + 1])].tobytes(), oblob[int(ooffs[i]):int(ooffs[i + 1])].tobytes()
            assert a == b, f"row {i}: {lines[i]!r}\n  gpu    {a!r}\n  oracle {b!r}"
    finally:
        d.close()


def test_decode_datagrams_returns_records_and_the_reference_errors(oracle):
    from flowgger_amd import DecodeError, Record

    d = RFC3164Decoder(RFC3164_CONFIG)
    cases = dict(um.case_list())
    res = d.decode_datagrams([cases["ref_raw"], cases["ref_zlib"], cases["ref_gzip"], cases["ref_gzip_trunc5"], cases["zlib_bad_adler"],
                              cases["gz_bad_crc32"], cases["match_past_cap"]], max_inflated=None)
    assert all(isinstance(r, Record) for r in res[:3]) and res[0] == res[1] == res[2]
    assert [str(r) for r in res[3:6]] == ["Invalid UTF-8 input", "Corrupted compressed (zlib) record", "Corrupted compressed (gzip) record"]
    assert isinstance(res[6], DecodeError)
    d.close()


def test_capnp_is_rejected():
    from flowgger_amd import CapnpDecoder

    d = CapnpDecoder()
    blob, offs = um.pack([b"abc"])
    st = L.fg_tables()
    a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
    rc = L.lib().fg_udp_decode_batch(d._ctx, L.FG_CAPNP, blob.ctypes.data, blob.size, offs.ctypes.data, 1, 0, C.byref(st), C.byref(a), C.byref(b),
                                     C.byref(c))
    assert rc == L.FG_ERR_ARG
    d.close()


def test_cpp_udp_batcher(tmp_path):
    """fg::UdpBatcher (host/fg_decoder.hpp) over several flushes: a Record or the reference's text per datagram, in arrival order"""
    import struct
    import subprocess
    from pathlib import Path

    from flowgger_amd import DecodeError

    root = Path(__file__).resolve().parent.parent
    exe = tmp_path / "udp_batcher_test"
    subprocess.run(["g++", "-std=c++17", "-O1", str(root / "tests/native/udp_batcher_test.cpp"), "-o", str(exe), f"-I{root / 'include'}",
                    f"-I{root / 'flowgger_amd/host'}", f"-L{root / 'flowgger_amd'}", "-lfg_hip", f"-Wl,-rpath,{root / 'flowgger_amd'}",
                    "-L/opt/rocm/lib", "-lamdhip64"], check=True)
    cases = dict(um.case_list(CAP))
    grams = datagrams_of(corpus(GELF, 600), 9) + [cases[k] for k in ("zlib_bad_adler", "gz_bad_crc32", "raw_bad_utf8", "match_past_cap", "empty")]
    (tmp_path / "grams.bin").write_bytes(b"".join(struct.pack("<I", len(g)) + g for g in grams))
    r = subprocess.run([str(exe), "run", str(tmp_path / "grams.bin"), "97"], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    d = GelfDecoder()
    want = []
    for res in d.decode_datagrams(grams, max_inflated=CAP):
        want.append(str(res).encode() if isinstance(res, DecodeError) else b"R\t" + res.hostname.encode() + b"\t%d" % len((res.msg or "").encode()))
    d.close()
    st, _, _ = um.expect(grams, CAP)
    want.append(b"too_large\t%d" % int((st == um.TOO_LARGE).sum()))
    assert int((st == um.TOO_LARGE).sum()) == 1 and sum(w == b"Corrupted compressed (zlib) record" for w in want) >= 1
    assert r.stdout.split(b"\n")[:-1] == want
