"""CPU: CapnpFramer (flowgger_amd/decoder.py) -- the framing half of CapnpSplitter::run: a Cap'n Proto stream is a chain of
length prefixes (capnp::serialize::read_message), walked on the host.  A stream cut at every byte position gives the offsets of
the whole stream; the two conditions under which read_message ends the connection are reported as such."""
import struct

import numpy as np
import pytest

import capnp_read_model as M
import capnp_wire as W
from flowgger_amd import CapnpFramer, CapnpStreamError
from flowgger_amd.record import Record, SDValue, StructuredData


def messages():
    recs = [Record(ts=1.5, hostname="a"), Record(ts=2.5, hostname="host", msg="m" * 30, sd=[StructuredData("id", [("k", SDValue("String", "v"))])]),
            Record(ts=3.5, hostname="h", full_msg="x" * 9000)]  # (the last one spans two segments)
    msgs = [W.serialize(r) for r in recs]
    msgs.append(struct.pack("<4I", 2, 1, 0, 2) + bytes(24))     # three segments, one of them empty
    msgs.append(struct.pack("<2I", 0, 0))                        # one empty segment: 8 bytes in all
    assert struct.unpack_from("<I", msgs[2])[0] == 1
    return msgs


def test_whole_stream_and_every_cut():
    msgs = messages()
    stream = b"".join(msgs)
    want = np.concatenate([[0], np.cumsum([len(m) for m in msgs])]).astype(np.uint64)
    offs, consumed = CapnpFramer.frame(stream)
    assert np.array_equal(offs, want) and consumed == len(stream)
    assert M.frame_stream(stream) == ([int(x) for x in want], len(stream), None)
    for cut in range(len(stream) + 1):
        f = CapnpFramer()
        d1, o1 = f.feed(stream[:cut])
        assert f.pending == cut - len(d1)
        d2, o2 = f.feed(stream[cut:])
        assert f.pending == 0
        got = np.concatenate([o1, o2[1:] + np.uint64(len(d1))])
        assert np.array_equal(got, want), cut
        assert d1.tobytes() + d2.tobytes() == stream
        assert all(int(x) % 8 == 0 for x in o1) and all(int(x) % 8 == 0 for x in o2)   # a message starts on a word
    # byte by byte
    f, seen = CapnpFramer(), 0
    for i in range(len(stream)):
        d, o = f.feed(stream[i:i + 1])
        seen += len(o) - 1
    assert seen == len(msgs) and f.pending == 0


def test_an_incomplete_tail_is_carried_not_framed():
    msgs = messages()
    f = CapnpFramer()
    d, o = f.feed(msgs[0] + msgs[1][:-1])
    assert len(o) == 2 and d.tobytes() == msgs[0] and f.pending == len(msgs[1]) - 1
    d, o = f.feed(b"")
    assert len(o) == 1 and d.size == 0


@pytest.mark.parametrize("head,ok", [(struct.pack("<2I", 510, 0) + bytes(4 * 510), True),     # 511 segments
                                     (struct.pack("<2I", 511, 0), False),                        # 512: "Too many segments"
                                     (struct.pack("<2I", 0xFFFFFFFF, 0), False),
                                     (struct.pack("<2I", 0, 8 << 20), True),                      # 8 Mi words: allowed (the body is not there yet)
                                     (struct.pack("<2I", 0, (8 << 20) + 1), False),               # one more: too large
                                     (struct.pack("<4I", 1, 8 << 20, 1, 0), False)])
def test_conditions_that_end_the_connection(head, ok):
    good = W.serialize(Record(ts=1.5, hostname="a"))
    f = CapnpFramer()
    if ok:
        d, o = f.feed(good + head)
        assert len(o) == 2 or (len(o) == 3 and struct.unpack_from("<I", head)[0] == 510)
        assert M.frame_stream(good + head)[2] is None
    else:
        # the reference handles the whole messages in front of the bad table first and ends the connection afterwards
        # (capnp_splitter.rs:24-60): feed() delivers them, the NEXT call raises; frame() puts them on the exception
        d, o = f.feed(good + head)
        assert d.tobytes() == good and [int(x) for x in o] == [0, len(good)]
        with pytest.raises(CapnpStreamError):
            f.feed(b"")
        with pytest.raises(CapnpStreamError):
            f.feed(good)                       # the connection stays ended
        with pytest.raises(CapnpStreamError) as e:
            CapnpFramer.frame(good + head)
        assert [int(x) for x in e.value.offsets] == [0, len(good)] and e.value.consumed == len(good)
        f2 = CapnpFramer()
        with pytest.raises(CapnpStreamError):  # nothing whole in front of it: raised at once
            f2.feed(head)
        offs, consumed, err = M.frame_stream(good + head)
        assert err is not None and offs == [0, len(good)] and consumed == len(good)


def test_the_cpp_framer_agrees():
    """CapnpFramer of flowgger_amd/host/fg_decoder.hpp: the same offsets, consumed bytes and verdicts as the model, at every cut"""
    import ctypes as C
    import subprocess
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    src, lib = root / "tests/native/capnp_framer_host.cpp", root / "tests/native/libcapnp_framer_host.so"
    deps = [src, root / "flowgger_amd/host/fg_decoder.hpp", root / "include/fg_hip.h"]
    if not lib.exists() or lib.stat().st_mtime < max(p.stat().st_mtime for p in deps):
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", str(lib), str(src)], check=True)
    h = C.CDLL(str(lib))

    def frame(buf):
        offs = np.zeros(64, np.uint64)
        cnt, cons = C.c_uint64(), C.c_uint64()
        st = h.fgc_frame(buf, C.c_uint64(len(buf)), C.c_void_p(offs.ctypes.data), C.c_uint64(64), C.byref(cnt), C.byref(cons))
        return st, [int(x) for x in offs[:cnt.value]], cons.value
    stream = b"".join(messages())
    for cut in range(len(stream) + 1):
        want = M.frame_stream(stream[:cut])
        assert frame(stream[:cut]) == (0, want[0], want[1]), cut
    good = W.serialize(Record(ts=1.5, hostname="a"))
    assert frame(good + struct.pack("<2I", 511, 0)) == (1, [0, len(good)], len(good))
    assert frame(good + struct.pack("<2I", 0, (8 << 20) + 1)) == (2, [0, len(good)], len(good))
    assert frame(good + struct.pack("<2I", 0, 8 << 20))[0] == 0
