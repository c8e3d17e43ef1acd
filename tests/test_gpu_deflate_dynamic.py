"""GPU: FG_DEFLATE_DYNAMIC (fg_set_deflate_mode; k_df_blocks_dyn of fg_deflate.hip) -- Encoder.deflate_device(huffman="dynamic") byte for
byte against the same core on the wave emulation (tests/deflate_dyn_model.py) and against zlib; Pipeline(huffman="dynamic") against
the plain run and the fixed-mode run; the dynamic members back through the project's own inflater."""
from __future__ import annotations

import ctypes as C
import zlib

import numpy as np
import pytest

import deflate_dyn_model as ddm
import deflate_model as dm
from flowgger_amd import Encoder, GelfDecoder, GelfEncoder, Pipeline, synth
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
    return ddm.DynHost()


def gpu_deflate(dec, members, **kw):
    import torch

    dev = torch.device("cuda", dec.device)
    blob, cuts = dm.pack_members(members)
    d_bytes = torch.from_numpy(blob[:int(cuts[-1])].copy()).to(dev)
    d_cuts = torch.from_numpy(cuts.astype(np.int64)).to(dev)
    d_z, d_zoff = Encoder.deflate_device(dec, d_bytes, d_cuts, **kw)
    torch.cuda.synchronize(dev)
    return d_z.cpu().numpy(), d_zoff.cpu().numpy().astype(np.uint64)


def test_case_list_and_named_shapes_equal_the_emulation(dec, host):
    B = host.block
    assert B == int(L.lib().fg_deflate_block_bytes())
    names, members = ddm.all_cases(B)
    z, zoffs = gpu_deflate(dec, members, huffman="dynamic")
    dm.check_members(members, z, zoffs, B, "dynamic")
    assert int(zoffs[-1]) <= int(L.lib().fg_deflate_bound(sum(map(len, members)), len(members)))
    hz = ddm.emulate(host, members, ddm.DYNAMIC)
    got = dm.split(z, zoffs)
    assert [n for n, a, b in zip(names, got, hz) if a != b] == []
    for n, zm in zip(names, got):
        if n.startswith("shape/"):
            assert ddm.btype(zm) == 2, n
    # the fixed mode named, the default, and the mode left behind by the call before
    z2, zoffs2 = gpu_deflate(dec, members, huffman="dynamic")
    assert np.array_equal(z, z2) and np.array_equal(zoffs, zoffs2)
    zf, zfoffs = gpu_deflate(dec, members, huffman="fixed")
    zd, zdoffs = gpu_deflate(dec, members)
    assert np.array_equal(zf, zd) and np.array_equal(zfoffs, zdoffs)
    assert dm.split(zf, zfoffs) == ddm.emulate(host, members, ddm.FIXED)
    assert (np.diff(zoffs.astype(np.int64)) <= np.diff(zfoffs.astype(np.int64))).all()
    with pytest.raises(ValueError):
        gpu_deflate(dec, members[:1], huffman="static")


POLICIES = [(1, 0), (0, 4096), (0, 65536)]


@pytest.fixture(scope="module")
def plain():
    d = GelfDecoder()
    try:
        lines = synth.gelf_lines(3000)
        return lines, Pipeline(d, GelfEncoder(None, merger="line")).run_packed(*synth.pack(lines), now_ts=NOW)
    finally:
        d.close()


@pytest.mark.parametrize("coalesce,member_bytes", POLICIES)
def test_pipeline_dynamic_equals_the_plain_stream(plain, coalesce, member_bytes):
    lines, w = plain
    data, offsets = synth.pack(lines)
    d = GelfDecoder()
    try:
        enc = GelfEncoder(None, merger="line")
        t = Pipeline(d, enc, compression="gzip", huffman="dynamic", coalesce=coalesce, member_bytes=member_bytes).run_packed(data, offsets, now_ts=NOW)
        f = Pipeline(d, enc, compression="gzip", huffman="fixed", coalesce=coalesce, member_bytes=member_bytes).run_packed(data, offsets, now_ts=NOW)
        assert t.out is None and t.raw_bytes == w.out.size > 100_000
        for k in ("out_offsets", "meta", "enc_status", ):
            assert np.array_equal(getattr(t, k), getattr(w, k)), k
        assert np.array_equal(t.member_first, f.member_first)
        first, cuts = dm.model_members(w.out_offsets, coalesce, member_bytes, int(L.lib().fg_deflate_block_bytes()))
        assert np.array_equal(t.member_first, first)
        assert b"".join(zlib.decompress(m, 31) for m in t.members() if m) == w.out.tobytes()
        assert b"".join(zlib.decompress(m, 31) for m in f.members() if m) == w.out.tobytes()
        print(f"coalesce {coalesce} member_bytes {member_bytes}: raw {w.out.size} fixed {f.z.size} dynamic {t.z.size}")
        assert t.z.size <= f.z.size
        assert any(ddm.btype(m) == 2 for m in t.members() if m) and not any(ddm.btype(m) == 2 for m in f.members() if m)
        # a plain Pipeline on the same ctx right after: the plain stream, no members
        p = Pipeline(d, enc).run_packed(data, offsets, now_ts=NOW)
        assert p.out.tobytes() == w.out.tobytes() and p.z is None
        c = L.fg_compressed()
        assert L.lib().fg_last_compressed(d._ctx, C.byref(c)) == L.FG_OK and c.n_members == 0 and c.z_bytes == 0 and not c.z
    finally:
        d.close()


def test_pipeline_refuses_another_mode():
    d = GelfDecoder()
    try:
        with pytest.raises(ValueError):
            Pipeline(d, GelfEncoder(None, merger="line"), compression="gzip", huffman="best")
        assert L.lib().fg_set_deflate_mode(d._ctx, 2) == L.FG_ERR_ARG and L.lib().fg_set_deflate_mode(None, 1) == L.FG_ERR_ARG
    finally:
        d.close()


def test_dynamic_members_through_the_projects_inflater(dec, host):
    import test_gpu_udp as TU
    import udp_model as um

    lines = synth.gelf_lines(600, invalid_frac=0)
    members = [b"\n".join(lines[k:k + 1 + k % 40]) for k in range(0, 560, 40)] + [m for _, m in ddm.named_shapes(host.block)]
    z, zoffs = gpu_deflate(dec, members, huffman="dynamic")
    grams = dm.split(z, zoffs)
    assert all(24 <= len(g) <= 65527 for g in grams) and all(ddm.btype(g) == 2 for g in grams)
    offs, packed, drop, st = TU.unpack(dec, grams, max(map(len, members)))
    assert st.tolist() == [um.GZIP] * len(members) and not drop.any()
    assert [bytes(packed[int(offs[k]):int(offs[k + 1])]) for k in range(len(members))] == members
