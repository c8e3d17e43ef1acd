"""CPU: the Cap'n Proto stream framer's device logic (flowgger_amd/csrc/fg_capnp_frame.hpp: mark, nodes, link, rank, emit) on the wave
emulation, and the sequential walk it shares with the host route (fg_capnp_next.hpp), against CapnpFramer.frame -- the restatement
of capnp::serialize::read_message as CapnpSplitter::run calls it (splitter/capnp_splitter.rs:24-46)."""
from __future__ import annotations

import json
import struct

import numpy as np
import pytest

import capnp_frame_binding as B
from capnp_frame_binding import CLEAN, TAIL, TOO_LARGE, TOO_MANY_SEGMENTS, CapnpFrameHost, model


@pytest.fixture(scope="module")
def host():
    return CapnpFrameHost()


def check(host, buf, may_decline=False):
    """the sequential walk and every run of the device logic reproduce the offsets, `consumed` and the stop of the model"""
    offs, consumed, stop = model(buf)
    assert host.walk(buf) == (offs, consumed, stop)
    r = host.frame(buf)
    if r["declined"]:
        assert may_decline, "the device logic declined"
        return None
    n = len(offs) - 1
    assert (r["n"], r["consumed"], r["stop"]) == (n, consumed, stop)
    assert [int(x) for x in r["offsets"]] == offs[:n] + [consumed]
    return r


def test_the_model_s_offsets_end_at_consumed():
    for buf in (b"", B.msg(0), B.msg(3) + b"abc"):
        offs, consumed, _ = model(buf)
        assert offs[-1] == consumed


def test_shapes(host):
    want = {"empty": CLEAN, "one_8_byte_message": CLEAN, "one_tile_long": CLEAN, "512_segments_behind_good": TOO_MANY_SEGMENTS,
            "sum_8mi_words_is_a_tail": TAIL, "sum_8mi_plus_1_is_too_large": TOO_LARGE, "tail_inside_the_table": TAIL,
            "tail_inside_the_body": TAIL, "511_segments": CLEAN, "3_bytes": TAIL, "7_bytes_behind_a_message": TAIL}
    sh = B.shapes(host.tile_words)
    for name, buf in sh.items():
        r = check(host, buf)
        if name in want:
            assert r["stop"] == want[name], name
    assert check(host, sh["512_segments_behind_good"])["n"] == 2          # the whole messages in front of the bad table are output
    assert check(host, sh["one_tile_long"])["consumed"] == host.tile_words * 8
    assert check(host, sh["one_8_byte_message"])["n"] == 1
    assert check(host, sh["511_segments"])["n"] == 3


def test_every_cut_of_a_small_stream(host):
    stream = B.msg(0) + B.msg(2, 1, fill=b"ab") + B.msg(7, fill=struct.pack("<2I", 0, 1)) + B.msg(1, 0, 2) + B.msg(0)
    for cut in range(len(stream) + 1):
        r = check(host, stream[:cut])
        assert r["stop"] in (CLEAN, TAIL)


def test_cap_frames_too_small_reports_the_need(host):
    buf = B.msg(0) * 700 + B.msg(600) + B.msg(3) * 5
    full = check(host, buf)
    r = host.frame(buf, cap=10)
    assert not r["declined"] and r["n"] == full["n"] == 706           # (the caller sees n > cap: FG_ERR_ENT_OVERFLOW)
    assert [int(x) for x in r["offsets"][:10]] == [int(x) for x in full["offsets"][:10]]
    r = host.frame(buf, cap=706)
    assert np.array_equal(r["offsets"], full["offsets"])


def test_seeded_fuzz_with_random_cuts(host):
    rng = np.random.default_rng(20261018)
    total = 0
    for _ in range(12):
        stream = B.fuzz_stream(rng, 300)
        total += 300
        check(host, stream)
        for _ in range(3):
            check(host, stream[:int(rng.integers(0, len(stream) + 1))])
    assert total >= 3000


def test_a_stream_beyond_the_node_store_declines(host):
    raw = B.node_heavy_stream()
    r = host.frame(raw)
    assert r["declined"] != 0 and r["nodes"] > host.node_cap(len(raw))
    offs, consumed, stop = model(raw)                                   # (the stream itself is fine: the caller walks it on the host)
    assert (len(offs) - 1, consumed, stop) == (3, len(raw), CLEAN)
    assert host.walk(raw) == (offs, consumed, stop)


# ---- the corpora that must not decline; the largest nodes per word seen is the measurement behind kNodeDiv (DESIGN) ----------------
def synth_messages(name, n):
    """the CORPORA of tests/test_gpu_capnp.py as the capnp encoder writes them: the oracle's Records through the wire model"""
    import capnp_wire as W
    import oracle_binding
    from flowgger_amd import synth, tzdb
    from flowgger_amd.record import DecodeError, parse_canonical
    from test_gpu_capnp import CORPORA, EXTRA, NOW
    src, make = CORPORA[name]
    lines = make()[:n]
    o = oracle_binding.Oracle()
    o.set_rfc3164(2026, tzdb.default_table())
    data, offsets = synth.pack(lines)
    blob, offs = o.decode_batch(src, data, offsets, synth.LTSV_CONFIG if src == 1 else None)
    out = []
    for i in range(len(lines)):
        r = parse_canonical(blob[int(offs[i]):int(offs[i + 1])].tobytes(), now=NOW)
        if not isinstance(r, DecodeError):
            out.append(W.serialize(r, sorted(EXTRA.items())))
    return out


CORPUS_NAMES = ["rfc5424", "rfc5424_sd", "gelf", "ltsv", "rfc3164", "rfc5424_long_tail", "ltsv_long_tail"]


def nodes_per_word(r, buf):
    return r["nodes"] / max(len(buf) // 8, 1)


@pytest.mark.parametrize("name", CORPUS_NAMES)
def test_encoder_corpora_never_decline(host, name):
    msgs = synth_messages(name, 400)
    assert len(msgs) > 300
    buf = b"".join(msgs)
    r = check(host, buf)
    assert r["stop"] == CLEAN and r["n"] == len(msgs)
    print(f"{name}: {len(buf)} bytes, {r['nodes']} nodes, {nodes_per_word(r, buf):.5f} per word")
    assert r["nodes"] * 4 <= host.node_cap(len(buf))                      # the 4x margin of the node store


def test_mutated_message_corpus_never_declines(host):
    from test_capnp_in_cpu import fuzz_corpus
    buf = b"".join(fuzz_corpus(1500, 20261016))
    r = check(host, buf)
    print(f"mutated: {len(buf)} bytes, {r['nodes']} nodes, {nodes_per_word(r, buf):.5f} per word")
    assert r["nodes"] * 4 <= host.node_cap(len(buf))


def test_reference_vector_repeated_never_declines(host):
    from capnp_frame_binding import ROOT
    v = bytes(json.loads((ROOT / "tests/golden/capnp_splitter_vector.json").read_text())["message"])
    buf = v * 700
    r = check(host, buf)
    assert (r["n"], r["stop"]) == (700, CLEAN)
    print(f"vector: {len(buf)} bytes, {r['nodes']} nodes, {nodes_per_word(r, buf):.5f} per word")
    assert r["nodes"] * 4 <= host.node_cap(len(buf))
