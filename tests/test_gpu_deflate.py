"""GPU: the output compressor (fg_deflate.hip) -- fg_deflate_device against Python's zlib and, byte for byte, against the same core on
the wave emulation (tests/deflate_model.py); Pipeline(compression="gzip") through every transcode entry point against the same call
without compression; the members back through the project's own inflater."""
from __future__ import annotations

import ctypes as C
import zlib

import numpy as np
import pytest

import deflate_model as dm
from flowgger_amd import Encoder, GelfDecoder, GelfEncoder, Pipeline, RFC5424Decoder, synth
from flowgger_amd import _lib as L

pytestmark = pytest.mark.gpu
NOW = 1_700_000_000.0


@pytest.fixture(scope="module")
def dec():
    d = GelfDecoder()
    yield d
    d.close()


@pytest.fixture(scope="module")
def host():
    return dm.DeflateHost()


@pytest.fixture(scope="module")
def block():
    return int(L.lib().fg_deflate_block_bytes())


def gpu_deflate(dec, members, out=None):
    import torch

    dev = torch.device("cuda", dec.device)
    blob, cuts = dm.pack_members(members)
    d_bytes = torch.from_numpy(blob[:int(cuts[-1])].copy()).to(dev)
    d_cuts = torch.from_numpy(cuts.astype(np.int64)).to(dev)
    d_z, d_zoff = Encoder.deflate_device(dec, d_bytes, d_cuts, out=out)
    torch.cuda.synchronize(dev)
    return d_z.cpu().numpy(), d_zoff.cpu().numpy().astype(np.uint64)


def test_block_bytes_and_bound(host, block):
    assert 16384 <= block <= 65535 and block == host.block
    for nbytes, nm in ((0, 0), (1, 1), (block, 1), (10 * block + 3, 7), (1 << 30, 1 << 20)):
        assert int(L.lib().fg_deflate_bound(nbytes, nm)) == host.bound(nbytes, nm) >= nbytes + 18 * nm


@pytest.fixture(scope="module")
def case_list(host, block):
    names, members = dm.case_members(block)
    members = members + dm.cross_cases(block)
    names = names + [f"cross/{k}" for k in range(len(members) - len(names))]
    z, zoffs = host.deflate(members)
    return names, members, z, zoffs


def test_case_list_inflates_and_equals_the_emulation(dec, block, case_list):
    names, members, hz, hzoffs = case_list
    z, zoffs = gpu_deflate(dec, members)
    dm.check_members(members, z, zoffs, block, "case list")
    assert np.array_equal(zoffs, hzoffs), [n for n, a, b in zip(names, np.diff(zoffs.astype(np.int64)), np.diff(hzoffs.astype(np.int64))) if a != b][:5]
    assert np.array_equal(z, hz)
    assert int(zoffs[-1]) <= int(L.lib().fg_deflate_bound(sum(map(len, members)), len(members)))
    # the same input again: the same bytes
    z2, zoffs2 = gpu_deflate(dec, members)
    assert np.array_equal(z, z2) and np.array_equal(zoffs, zoffs2)


def test_equal_members_and_empty_ones(dec, host, block):
    members = dm.equal_members(40)
    z, zoffs = gpu_deflate(dec, members)
    dm.check_members(members, z, zoffs, block, "40 equal members")
    hz, hzoffs = host.deflate(members)
    assert np.array_equal(z, hz) and np.array_equal(zoffs, hzoffs)
    assert len(set(dm.split(z, zoffs))) == 1  # (a member that saw its neighbour would differ from the first)
    mixed = [b"", b"", members[0], b"", b"", b"x", members[0][:100], b"", b""]
    z, zoffs = gpu_deflate(dec, mixed)
    dm.check_members(mixed, z, zoffs, block, "empty and non-empty members")
    hz, hzoffs = host.deflate(mixed)
    assert np.array_equal(z, hz) and np.array_equal(zoffs, hzoffs)
    assert [int(zoffs[k + 1] - zoffs[k]) == 0 for k in range(len(mixed))] == [not m for m in mixed]


def test_sizing_call_overflow_and_no_members(dec, block):
    import torch

    dev = torch.device("cuda", dec.device)
    members = [b"\n".join(synth.gelf_lines(60)), b"", bytes(range(256)) * 10, b"q" * 700]
    blob, cuts = dm.pack_members(members)
    n, nbytes = len(members), int(cuts[-1])
    d_bytes = torch.from_numpy(blob[:nbytes].copy()).to(dev)
    d_cuts = torch.from_numpy(cuts.astype(np.int64)).to(dev)
    d_zoff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    total = C.c_uint64()
    lib = L.lib()
    head = (dec._ctx, d_bytes.data_ptr(), nbytes, d_cuts.data_ptr(), n)
    tail = (d_zoff.data_ptr(), C.byref(total), None)
    assert lib.fg_deflate_device(*head, None, 0, *tail) == L.FG_OK
    need = int(total.value)
    sized = d_zoff.cpu().numpy().copy()
    assert 0 < need < nbytes and int(sized[-1]) == need
    d_z = torch.full((need + 64,), 0xEE, dtype=torch.uint8, device=dev)
    assert lib.fg_deflate_device(*head, d_z.data_ptr(), need - 1, *tail) == L.FG_ERR_ENT_OVERFLOW and int(total.value) == need
    torch.cuda.synchronize(dev)
    assert bool((d_z == 0xEE).all()), "an overflowing call wrote member bytes"
    assert lib.fg_deflate_device(*head, d_z.data_ptr(), need, *tail) == L.FG_OK and int(total.value) == need
    torch.cuda.synchronize(dev)
    out = d_z.cpu().numpy()
    assert bool((out[need:] == 0xEE).all()), "bytes written behind the last member"
    assert np.array_equal(d_zoff.cpu().numpy(), sized)
    dm.check_members(members, out[:need], d_zoff.cpu().numpy().astype(np.uint64), block, "exact capacity")
    # no members at all
    d_zoff.fill_(7)
    assert lib.fg_deflate_device(dec._ctx, d_bytes.data_ptr(), nbytes, d_cuts.data_ptr(), 0, None, 0, *tail) == L.FG_OK
    assert int(total.value) == 0 and int(d_zoff[0]) == 0
    # cuts that do not ascend, cuts beyond the buffer
    for bad in ([0, 10, 5, nbytes], [0, 10, nbytes + 1]):
        d_bad = torch.tensor(bad, dtype=torch.int64, device=dev)
        assert lib.fg_deflate_device(dec._ctx, d_bytes.data_ptr(), nbytes, d_bad.data_ptr(), len(bad) - 1, None, 0, *tail) == L.FG_ERR_ARG
    assert lib.fg_deflate_device(None, d_bytes.data_ptr(), nbytes, d_cuts.data_ptr(), n, None, 0, *tail) == L.FG_ERR_ARG


def test_many_more_blocks_than_waves(dec, host, block):
    rng = np.random.default_rng(11)
    text = b"\n".join(synth.gelf_lines(400))
    members = []
    for k in range(2000):
        n, a = int(rng.integers(1, 301)), int(rng.integers(0, len(text) - 300))
        members.append(text[a:a + n] if k % 3 else rng.integers(0, 256, n, dtype=np.uint8).tobytes())
    # (2000 blocks: more than the nine waves a CU holds on any part with fewer than 222 CUs -- the ticket path either way)
    z, zoffs = gpu_deflate(dec, members)
    dm.check_members(members, z, zoffs, block, "2000 small members")
    hz, hzoffs = host.deflate(members)
    assert np.array_equal(z, hz) and np.array_equal(zoffs, hzoffs)


def test_one_member_of_many_blocks(dec, host, block):
    lines = synth.gelf_lines(4000)
    raw = b"\n".join(lines)
    rng = np.random.default_rng(3)
    member = (raw[:2 * block] + rng.integers(0, 256, block, dtype=np.uint8).tobytes() + raw)[:5 * block + 7]
    assert len(member) == 5 * block + 7
    z, zoffs = gpu_deflate(dec, [member])
    dm.check_members([member], z, zoffs, block, "5B + 7")
    hz, hzoffs = host.deflate([member])
    assert np.array_equal(z, hz) and np.array_equal(zoffs, hzoffs)
    assert bytes(z).count(b"\x00\x00\xff\xff") >= 3  # (fixed blocks that are not the last end in a sync flush)


def test_round_trip_through_the_projects_inflater(dec, block):
    import test_gpu_udp as TU
    import udp_model as um

    lines = synth.gelf_lines(600, invalid_frac=0)
    members = [b"\n".join(lines[k:k + 1 + k % 40]) for k in range(0, 560, 40)] + [b"a" * 60000, bytes(range(32, 127)) * 600]
    z, zoffs = gpu_deflate(dec, members)
    grams = dm.split(z, zoffs)
    assert all(24 <= len(g) <= 65527 for g in grams)
    offs, packed, drop, st = TU.unpack(dec, grams, max(map(len, members)))
    assert st.tolist() == [um.GZIP] * len(members) and not drop.any()
    assert [bytes(packed[int(offs[k]):int(offs[k + 1])]) for k in range(len(members))] == members


# ---- Pipeline(compression="gzip") -----------------------------------------------------------------------------------------------------
CORPORA = {"rfc5424": (RFC5424Decoder, lambda: synth.rfc5424_lines(3000, cfg=2)), "gelf": (GelfDecoder, lambda: synth.gelf_lines(3000))}
POLICIES = [(1, 0), (7, 0), (4096, 0), (0, 0), (0, 4096)]


def runs(p, lines):
    """the four entry shapes over one corpus: name -> result"""
    data, offsets = synth.pack(lines)
    stream = b"\n".join(lines)  # (an unterminated tail)
    thirds = [b"\n".join(lines[k::3]) + (b"\n" if k != 1 else b"") for k in range(3)]
    starts = np.cumsum([0] + [len(t) for t in thirds]).astype(np.uint64)
    return {"packed": p.run_packed(data, offsets, now_ts=NOW),
            "stream_final": p.run_stream(stream, L.FG_FRAME_LINE, final=True, now_ts=NOW),
            "stream_open": p.run_stream(stream, L.FG_FRAME_LINE, final=False, now_ts=NOW),
            "multi": p.run_multi(b"".join(thirds), starts, [0, 1, 0], L.FG_FRAME_LINE, now_ts=NOW),
            "datagrams": p.run_datagrams([zlib.compress(x) if i % 3 == 0 else x for i, x in enumerate(lines)], now_ts=NOW)}


@pytest.fixture(scope="module")
def plain():
    out = {}
    for name, (make, corpus) in CORPORA.items():
        d = make()
        try:
            lines = corpus()
            out[name] = (lines, runs(Pipeline(d, GelfEncoder(None, merger="line")), lines))
        finally:
            d.close()
    return out


@pytest.mark.parametrize("coalesce,member_bytes", POLICIES)
@pytest.mark.parametrize("corpus", sorted(CORPORA))
def test_pipeline_gzip_equals_the_plain_stream(plain, block, corpus, coalesce, member_bytes):
    lines, want = plain[corpus]
    d = CORPORA[corpus][0]()
    try:
        got = runs(Pipeline(d, GelfEncoder(None, merger="line"), compression="gzip", coalesce=coalesce, member_bytes=member_bytes), lines)
        for shape, t in got.items():
            w = want[shape]
            tag = f"{corpus} {shape} coalesce={coalesce} member_bytes={member_bytes}"
            assert w.out is not None and w.out.size > 100_000 and w.z is None, tag
            assert t.out is None and t.raw_bytes == w.out.size, tag
            assert np.array_equal(t.out_offsets, w.out_offsets) and np.array_equal(t.meta, w.meta) and np.array_equal(t.enc_status, w.enc_status), tag
            assert int((t.enc_status != 0).sum()) >= 10, tag  # (the corpus' invalid lines: empty messages inside the members)
            members = t.members()
            first, cuts = dm.model_members(w.out_offsets, coalesce, member_bytes, block)
            assert np.array_equal(t.member_first, first), tag
            raw = [w.out[int(cuts[k]):int(cuts[k + 1])].tobytes() for k in range(len(cuts) - 1)]
            dm.check_members(raw, t.z, t.z_offsets, block, tag)
            assert b"".join(zlib.decompress(m, 31) for m in members if m) == w.out.tobytes(), tag
            assert t.messages() == [w.message(i) for i in range(w.n)], tag
            if coalesce != 1:  # (a member per 300-byte message pays more for its frame than fixed codes save)
                assert t.z.size < 0.8 * w.out.size, tag
        # the same ctx without compression right after: the plain stream again, and no members reported
        t = Pipeline(d, GelfEncoder(None, merger="line")).run_packed(*synth.pack(lines), now_ts=NOW)
        assert t.out.tobytes() == want["packed"].out.tobytes() and t.z is None
        c = L.fg_compressed()
        assert L.lib().fg_last_compressed(d._ctx, C.byref(c)) == L.FG_OK and c.n_members == 0 and c.z_bytes == 0 and not c.z
    finally:
        d.close()


def test_from_config():
    d = GelfDecoder()
    try:
        enc = GelfEncoder(None, merger="line")
        p = Pipeline.from_config(d, enc, {"output": {"kafka_compression": "GZip", "kafka_coalesce": 5}})
        assert p.compression == L.FG_COMP_GZIP and p.coalesce == 5
        lines = synth.gelf_lines(23, invalid_frac=0)
        t = p.run_packed(*synth.pack(lines), now_ts=NOW)
        assert t.out is None and len(t.members()) == 5 and t.member_first.tolist() == [0, 5, 10, 15, 20, 23]
        assert t.messages() == [Pipeline(d, enc).run_packed(*synth.pack(lines), now_ts=NOW).message(i) for i in range(23)]
        assert Pipeline.from_config(d, enc, {}).compression == L.FG_COMP_NONE and Pipeline.from_config(d, enc, {"output": {"kafka_compression": "NONE"}}).coalesce == 1
        with pytest.raises(NotImplementedError):
            Pipeline.from_config(d, enc, {"output": {"kafka_compression": "snappy"}})
        with pytest.raises(ValueError, match="Unsupported compression method"):
            Pipeline.from_config(d, enc, {"output": {"kafka_compression": "lz4"}})
    finally:
        d.close()
