"""CPU: Kafka v0 message sets behind the transcode entry points (fg_set_output_wire, fg_kafka_messageset_device, fg_kafka_wrap_device: the
host side in flowgger_amd/csrc/fg_capi.cpp and fg_host_pipeline.cpp) on the fake runtime of test_host_pipeline_cpu.py, built with host
loops over fg_kafka.hpp and fg_deflate.hpp in the place of the kernels (tests/native/host_pipeline_fake_kafka.cpp).  The cores are the
real ones, so what comes out is held against tests/kafka_wire.py and zlib; the decode and the encoder behind them are the fakes of
host_pipeline_fake.cpp, as in test_deflate_host_cpu.py, whose batches and entry points these tests share."""
import ctypes as C
import subprocess
import warnings

import numpy as np
import pytest

import deflate_model as dm
import kafka_model as km
import kafka_wire as kw
import test_deflate_dynamic_host_cpu as Y
import test_deflate_host_cpu as D
import test_host_pipeline_cpu as H
from flowgger_amd import _lib as L
from test_host_pipeline_cpu import Ctx

u64, vp = C.c_uint64, C.c_void_p
LIB = H.HERE / "libhost_pipeline_fake_kafka.so"
SRC = [H.HERE / "host_pipeline_fake_kafka.cpp", H.HERE / "kafka_driver.hpp", D.CSRC / "fg_kafka.hpp"] + D.SRC
POLICIES = D.POLICIES
assert POLICIES == [(1, 0), (7, 0), (4096, 0), (0, 0), (0, 4096)]
RAW, KAFKA = L.FG_WIRE_RAW, L.FG_WIRE_KAFKA_V0


@pytest.fixture(scope="module")
def fake():
    if not LIB.exists() or any(s.stat().st_mtime > LIB.stat().st_mtime for s in SRC):
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                        "-Wno-unused-variable", f"-I{H.HERE / 'fakehip'}", f"-I{H.ROOT / 'include'}", f"-I{D.CSRC}", f"-I{H.HERE}", "-o", str(LIB), str(SRC[0])],
                       check=True)
    lib = C.CDLL(str(LIB))
    lib.fg_create.argtypes = [C.c_int, vp, C.POINTER(vp)]
    lib.fg_destroy.argtypes = [vp]
    lib.fg_destroy.restype = None
    lib.fg_clone.argtypes = [vp, C.POINTER(vp)]
    lib.fg_last_hip_error.argtypes = [vp]
    lib.fg_transcode_batch.argtypes = [vp, C.c_int, C.c_int, C.POINTER(L.fg_encode_cfg), vp, u64, vp, u64, C.c_int, C.POINTER(L.fg_transcoded)]
    lib.fg_transcode_multi_batch.argtypes = [vp, C.c_int, C.c_int, C.POINTER(L.fg_encode_cfg), vp, u64, vp, vp, u64, C.POINTER(L.fg_transcoded_multi)]
    lib.fg_udp_transcode_batch.argtypes = [vp, C.c_int, C.POINTER(L.fg_encode_cfg), vp, u64, vp, u64, u64, C.POINTER(L.fg_transcoded), C.POINTER(vp)]
    lib.fg_set_output_compression.argtypes = [vp, C.POINTER(L.fg_compress_cfg)]
    lib.fg_last_compressed.argtypes = [vp, C.POINTER(L.fg_compressed)]
    lib.fg_set_output_wire.argtypes = [vp, C.c_int]
    lib.fg_kafka_messageset_device.argtypes = [vp, vp, u64, vp, vp, u64, vp, u64, vp, C.POINTER(u64), vp]
    lib.fg_kafka_wrap_device.argtypes = [vp, vp, vp, u64, vp, u64, vp, C.POINTER(u64), vp]
    lib.fg_kafka_bound.argtypes = [u64, u64, u64]
    lib.fg_kafka_bound.restype = u64
    lib.fg_kafka_message_overhead.restype = C.c_uint32
    lib.fg_deflate_block_bytes.restype = C.c_uint32
    lib.fgf_fail_call_after.argtypes = [C.c_longlong]
    lib.fgf_calls.restype = lib.fgf_in_flight.restype = C.c_ulonglong
    lib.fgf_ctx_wire.argtypes = [vp]
    return lib


def kafka_launches(lib, reset=True):
    a = (C.c_ulonglong * 5)()
    lib.fgf_kafka_launches(a, int(reset))
    return [int(x) for x in a]


def set_wire(lib, ctx, wire):
    assert lib.fg_set_output_wire(ctx.h, wire) == 0


@pytest.mark.parametrize("coalesce,member_bytes", POLICIES)
@pytest.mark.parametrize("codec", ["none", "gzip"])
@pytest.mark.parametrize("entry", sorted(D.ENTRIES))
def test_message_sets_in_the_place_of_the_stream(fake, entry, codec, coalesce, member_bytes):
    B = int(fake.fg_deflate_block_bytes())
    run = D.ENTRIES[entry]
    lines = D.lines_of(300)
    c = Ctx(fake)
    rc, out, n = run(fake, c, lines)
    assert rc == 0
    plain = D.result(out, n)
    messages = [plain["out"][int(a):int(b)] for a, b in zip(plain["out_offsets"][:-1], plain["out_offsets"][1:])]
    failed = plain["enc_status"] != 0
    assert failed.sum() >= 3 and all(not messages[i] for i in np.flatnonzero(failed))
    # the parent's members on this ctx, to come back to
    D.set_compression(fake, c, L.FG_COMP_GZIP if codec == "gzip" else L.FG_COMP_NONE, coalesce, member_bytes)
    rc, out, _ = run(fake, c, lines)
    assert rc == 0
    before = (D.result(out, n)["out"], D.compressed(fake, c))
    set_wire(fake, c, KAFKA)
    assert run(fake, c, lines)[0] == 0  # (the buffers exist from here on)
    kafka_launches(fake)
    D.launches(fake)
    rc, out, n2 = run(fake, c, lines)
    assert rc == 0 and fake.fgf_in_flight() == 0 and n2 == n
    gz = codec == "gzip"
    assert kafka_launches(fake) == [1, 1, 1, int(gz), int(gz)] and D.launches(fake) == [1] + [int(gz)] * 4
    got = D.result(out, n)
    assert got["out"] is None and got["out_bytes"] == len(plain["out"]) > 10_000
    for k in ("out_offsets", "meta", "enc_status"):
        assert np.array_equal(got[k], plain[k]), k
    z = D.compressed(fake, c)
    first, _ = dm.model_members(plain["out_offsets"], coalesce, member_bytes, B)
    nm = len(first) - 1
    assert np.array_equal(z["member_first"], first) and z["n_members"] == nm and z["raw_bytes"] == len(plain["out"])
    zo = z["z_offsets"]
    assert int(zo[0]) == 0 and int(zo[-1]) == len(z["z"]) and (np.diff(zo.astype(np.int64)) >= 0).all()
    assert len(z["z"]) <= int(fake.fg_kafka_bound(len(plain["out"]), n, nm))
    seen = []
    for k, member in enumerate(dm.split(z["z"], zo)):
        rows = [i for i in range(int(first[k]), int(first[k + 1])) if not failed[i]]
        if not rows:
            assert member == b"", k
            continue
        if gz:
            wrappers = kw.parse_set(member)
            assert len(wrappers) == 1 and wrappers[0][0] and wrappers[0][1] == kw.ATTR_GZIP and wrappers[0][2][:10] == dm.HEADER, k
        else:
            assert member == kw.message_set([messages[i] for i in rows]), k
        recs = kw.records(member)
        assert recs == [(True, messages[i]) for i in rows], k
        seen += rows
    assert seen == [i for i in range(n) if not failed[i]]
    # ... and back to FG_WIRE_RAW on the same ctx: the parent's bytes
    set_wire(fake, c, RAW)
    rc, out, _ = run(fake, c, lines)
    after = (D.result(out, n)["out"], D.compressed(fake, c))
    assert rc == 0 and after[0] == before[0] and after[1]["n_members"] == before[1]["n_members"]
    for k in ("z", "z_offsets", "member_first"):
        assert np.array_equal(after[1][k], before[1][k]), k
    assert kafka_launches(fake) == [0] * 5
    c.close()


def test_nothing_but_dropped_lines_and_an_empty_batch(fake):
    for codec in (L.FG_COMP_GZIP, L.FG_COMP_NONE):
        c = Ctx(fake)
        D.set_compression(fake, c, codec, 2)
        set_wire(fake, c, KAFKA)
        rc, out, n = D.run_packed(fake, c, [b"", b"", b""])
        assert rc == 0 and int(out.out_bytes) == 0 and not out.out
        z = D.compressed(fake, c)
        assert z["n_members"] == 2 and z["z"].size == 0 and z["z_offsets"].tolist() == [0, 0, 0] and z["member_first"].tolist() == [0, 2, 3]
        rc, out, n = D.run_packed(fake, c, [b"a=1"])
        z = D.compressed(fake, c)
        assert rc == 0 and z["n_members"] == 1 and kw.records(z["z"].tobytes()) == [(True, b"a=1#\n")]
        rc, out, n = D.run_udp(fake, c, [])
        assert rc == 0 and D.compressed(fake, c)["n_members"] == 0
        c.close()


def test_the_setting_its_errors_and_its_clone(fake):
    c = Ctx(fake)
    assert fake.fgf_ctx_wire(c.h) == RAW
    assert fake.fg_set_output_wire(None, KAFKA) == L.FG_ERR_ARG
    for bad in (-1, 2, 7):
        assert fake.fg_set_output_wire(c.h, bad) == L.FG_ERR_ARG and fake.fgf_ctx_wire(c.h) == RAW
    set_wire(fake, c, KAFKA)
    twin = vp()
    assert fake.fg_clone(c.h, C.byref(twin)) == 0 and fake.fgf_ctx_wire(twin) == KAFKA
    fake.fg_destroy(twin)
    set_wire(fake, c, RAW)
    assert fake.fg_clone(c.h, C.byref(twin)) == 0 and fake.fgf_ctx_wire(twin) == RAW
    fake.fg_destroy(twin)
    assert int(fake.fg_kafka_message_overhead()) == kw.OVERHEAD
    c.close()


def test_argument_errors_of_the_resident_calls(fake):
    """host arrays play the device"""
    c = Ctx(fake)
    values = [b"k=v " * 100, b"", bytes(range(256)) * 3, b"x"]
    blob, off = km.pack(values)
    nbytes, n = int(off[-1]), len(values)
    skip = np.array([0, 0, 1, 0], np.uint8)
    so, total = np.zeros(n + 1, np.uint64), u64()
    call = fake.fg_kafka_messageset_device
    tail = (so.ctypes.data, C.byref(total), vp(-1))
    args = (blob.ctypes.data, nbytes, off.ctypes.data, skip.ctypes.data, n)
    assert call(None, *args, None, 0, *tail) == L.FG_ERR_ARG
    assert call(c.h, None, nbytes, *args[2:], None, 0, *tail) == L.FG_ERR_ARG
    assert call(c.h, blob.ctypes.data, nbytes, None, None, n, None, 0, *tail) == L.FG_ERR_ARG
    assert call(c.h, *args, None, 0, None, C.byref(total), vp(-1)) == L.FG_ERR_ARG
    assert call(c.h, *args, None, 0, so.ctypes.data, None, vp(-1)) == L.FG_ERR_ARG
    for bad in ([0, 500, 400, nbytes, nbytes], [0, 400, 400, 400, nbytes + 1], [5, 4, 4, 4, 4]):
        b = np.array(bad, np.uint64)
        assert call(c.h, blob.ctypes.data, nbytes, b.ctypes.data, None, n, None, 0, *tail) == L.FG_ERR_ARG and int(total.value) == 0, bad
    huge = np.array([0, 2**31 - 26], np.uint64)  # (only the sizes are looked at in a sizing call: the message would not fit int32)
    assert call(c.h, blob.ctypes.data, 2**33, huge.ctypes.data, None, 1, None, 0, *tail) == L.FG_ERR_ARG
    assert call(c.h, *args, None, 0, *tail) == 0 and fake.fgf_in_flight() == 0
    need = int(total.value)
    want = kw.message_set(values, skip)
    assert need == len(want) and so.tolist() == kw.set_offsets(values, skip)
    out = km.aligned(need + 8, 0xEE)
    assert call(c.h, *args, out.ctypes.data, need - 1, *tail) == L.FG_ERR_ENT_OVERFLOW and int(total.value) == need and (out == 0xEE).all()
    assert call(c.h, *args, out.ctypes.data, need, *tail) == 0 and (out[need:] == 0xEE).all() and out[:need].tobytes() == want
    full = kw.message_set(values)
    out = km.aligned(len(full) + 8, 0xEE)
    assert call(c.h, blob.ctypes.data, nbytes, off.ctypes.data, None, n, out.ctypes.data, len(full), *tail) == 0  # (d_skip NULL: every row)
    assert out[:len(full)].tobytes() == full and (out[len(full):] == 0xEE).all()
    so[:] = 9
    assert call(c.h, *args[:4], 0, None, 0, *tail) == 0 and int(so[0]) == 0 and int(total.value) == 0
    # fg_kafka_wrap_device
    members = km.wrap_members()
    z, zo = km.pack(members)
    nm = len(members)
    wo = np.zeros(nm + 1, np.uint64)
    wrap = fake.fg_kafka_wrap_device
    wtail = (wo.ctypes.data, C.byref(total), vp(-1))
    assert wrap(None, z.ctypes.data, zo.ctypes.data, nm, None, 0, *wtail) == L.FG_ERR_ARG
    assert wrap(c.h, z.ctypes.data, None, nm, None, 0, *wtail) == L.FG_ERR_ARG
    assert wrap(c.h, z.ctypes.data, zo.ctypes.data, nm, None, 0, None, C.byref(total), vp(-1)) == L.FG_ERR_ARG
    assert wrap(c.h, z.ctypes.data, zo.ctypes.data, nm, None, 0, wo.ctypes.data, None, vp(-1)) == L.FG_ERR_ARG
    down = np.array([0, 9, 5], np.uint64)
    assert wrap(c.h, z.ctypes.data, down.ctypes.data, 2, None, 0, *wtail) == L.FG_ERR_ARG
    assert wrap(c.h, z.ctypes.data, zo.ctypes.data, nm, None, 0, *wtail) == 0 and fake.fgf_in_flight() == 0
    need = int(total.value)
    want = km.expect_wrapped(members)
    assert need == len(want)
    out = km.aligned(need + 8, 0xEE)
    assert wrap(c.h, z.ctypes.data, zo.ctypes.data, nm, out.ctypes.data, need - 1, *wtail) == L.FG_ERR_ENT_OVERFLOW and (out == 0xEE).all()
    assert wrap(c.h, z.ctypes.data, zo.ctypes.data, nm, out.ctypes.data, need, *wtail) == 0 and (out[need:] == 0xEE).all() and out[:need].tobytes() == want
    wo[:] = 9
    assert wrap(c.h, z.ctypes.data, zo.ctypes.data, 0, None, 0, *wtail) == 0 and int(wo[0]) == 0 and int(total.value) == 0
    c.close()


def runtime_calls_and_caps(lib, entry, wire, codec, policy, dynamic=False):
    """the counted runtime calls of the first and of the second (warm) call of one configuration over D.lines_of(300) on a ctx of its
    own, and what fgf_deflate_caps reports behind them: d_df_slots, d_zout, h_zout, d_df_cut"""
    c = Ctx(lib)
    D.set_compression(lib, c, L.FG_COMP_GZIP if codec == "gzip" else L.FG_COMP_NONE, *policy)
    set_wire(lib, c, KAFKA if wire == "kafka" else RAW)
    if dynamic:
        assert lib.fg_set_deflate_mode(c.h, L.FG_DEFLATE_DYNAMIC) == 0
    lines, calls = D.lines_of(300), []
    for _ in range(2):
        c0 = lib.fgf_calls()
        assert D.ENTRIES[entry](lib, c, lines)[0] == 0 and lib.fgf_in_flight() == 0
        calls.append(int(lib.fgf_calls() - c0))
    caps = (C.c_ulonglong * 4)()
    lib.fgf_deflate_caps(c.h, caps)
    c.close()
    assert all(int(x) % (1 << 20) == 0 for x in caps)  # (grow_dev and grow_pinned round up to whole MiB)
    return calls + [int(x) >> 20 for x in caps]


# Recorded from the PARENT commit's fake build (compress_stage and kafka_stage as two functions, the resident entries written out one
# by one), not from the code under test: [calls of the first call, calls of the warm call, then the four capacities in MiB].
PARENT_CALLS_AND_CAPS = {
    ('multi', 'raw', 'none', 'fixed', (1, 0)): [27, 27, 0, 0, 0, 0],
    ('multi', 'raw', 'none', 'fixed', (0, 4096)): [27, 27, 0, 0, 0, 0],
    ('multi', 'raw', 'gzip', 'fixed', (1, 0)): [41, 41, 1, 1, 1, 1],
    ('multi', 'raw', 'gzip', 'fixed', (0, 4096)): [41, 41, 1, 1, 1, 1],
    ('multi', 'kafka', 'none', 'fixed', (1, 0)): [38, 38, 0, 0, 1, 1],
    ('multi', 'kafka', 'none', 'fixed', (0, 4096)): [38, 38, 0, 0, 1, 1],
    ('multi', 'kafka', 'gzip', 'fixed', (1, 0)): [53, 53, 1, 1, 1, 1],
    ('multi', 'kafka', 'gzip', 'fixed', (0, 4096)): [53, 53, 1, 1, 1, 1],
    ('multi', 'raw', 'gzip', 'dynamic', (1, 0)): [41, 41, 1, 1, 1, 1],
    ('multi', 'raw', 'gzip', 'dynamic', (0, 4096)): [41, 41, 1, 1, 1, 1],
    ('packed', 'raw', 'none', 'fixed', (1, 0)): [19, 19, 0, 0, 0, 0],
    ('packed', 'raw', 'none', 'fixed', (0, 4096)): [19, 19, 0, 0, 0, 0],
    ('packed', 'raw', 'gzip', 'fixed', (1, 0)): [33, 33, 1, 1, 1, 1],
    ('packed', 'raw', 'gzip', 'fixed', (0, 4096)): [33, 33, 1, 1, 1, 1],
    ('packed', 'kafka', 'none', 'fixed', (1, 0)): [30, 30, 0, 0, 1, 1],
    ('packed', 'kafka', 'none', 'fixed', (0, 4096)): [30, 30, 0, 0, 1, 1],
    ('packed', 'kafka', 'gzip', 'fixed', (1, 0)): [45, 45, 1, 1, 1, 1],
    ('packed', 'kafka', 'gzip', 'fixed', (0, 4096)): [45, 45, 1, 1, 1, 1],
    ('packed', 'raw', 'gzip', 'dynamic', (1, 0)): [33, 33, 1, 1, 1, 1],
    ('packed', 'raw', 'gzip', 'dynamic', (0, 4096)): [33, 33, 1, 1, 1, 1],
    ('udp', 'raw', 'none', 'fixed', (1, 0)): [27, 27, 0, 0, 0, 0],
    ('udp', 'raw', 'none', 'fixed', (0, 4096)): [27, 27, 0, 0, 0, 0],
    ('udp', 'raw', 'gzip', 'fixed', (1, 0)): [41, 41, 1, 1, 1, 1],
    ('udp', 'raw', 'gzip', 'fixed', (0, 4096)): [41, 41, 1, 1, 1, 1],
    ('udp', 'kafka', 'none', 'fixed', (1, 0)): [38, 38, 0, 0, 1, 1],
    ('udp', 'kafka', 'none', 'fixed', (0, 4096)): [38, 38, 0, 0, 1, 1],
    ('udp', 'kafka', 'gzip', 'fixed', (1, 0)): [53, 53, 1, 1, 1, 1],
    ('udp', 'kafka', 'gzip', 'fixed', (0, 4096)): [53, 53, 1, 1, 1, 1],
    ('udp', 'raw', 'gzip', 'dynamic', (1, 0)): [41, 41, 1, 1, 1, 1],
    ('udp', 'raw', 'gzip', 'dynamic', (0, 4096)): [41, 41, 1, 1, 1, 1],
}


@pytest.mark.parametrize("entry", sorted(D.ENTRIES))
def test_runtime_calls_and_capacities_are_the_parents(fake, entry):
    """every transcode entry, wire, codec and member policy (and FG_DEFLATE_DYNAMIC where a fake has its launcher: the library of
    test_deflate_dynamic_host_cpu.py, which has no Kafka launchers) makes the runtime calls the parent made and grows the compressor's
    buffers to the parent's sizes.  What this does not see: kafka with dynamic deflate (no fake library has both sets of launchers;
    the stand-alone program of the test below defines the missing one and runs those cells), and a layout whose byte count moves by
    less than the MiB the capacities are rounded to -- that is the stand-alone program's business too, under AddressSanitizer."""
    got = {}
    for wire in ("raw", "kafka"):
        for codec in ("none", "gzip"):
            for policy in ((1, 0), (0, 4096)):
                got[(entry, wire, codec, "fixed", policy)] = runtime_calls_and_caps(fake, entry, wire, codec, policy)
    dyn = Y.load(Y.LIB, Y.SRC)
    dyn.fg_set_output_wire.argtypes = [vp, C.c_int]
    dyn.fgf_deflate_caps.argtypes = [vp, C.POINTER(C.c_ulonglong)]
    for policy in ((1, 0), (0, 4096)):
        got[(entry, "raw", "gzip", "dynamic", policy)] = runtime_calls_and_caps(dyn, entry, "raw", "gzip", policy, dynamic=True)
    want = {k: v for k, v in PARENT_CALLS_AND_CAPS.items() if k[0] == entry}
    assert got == want


@pytest.mark.parametrize("codec", ["none", "gzip"])
@pytest.mark.parametrize("entry", sorted(D.ENTRIES))
def test_a_failed_runtime_call_at_every_index_leaves_nothing_in_flight_and_the_ctx_usable(fake, entry, codec):
    run = D.ENTRIES[entry]
    lines = D.lines_of(120)
    c = Ctx(fake)
    D.set_compression(fake, c, L.FG_COMP_GZIP if codec == "gzip" else L.FG_COMP_NONE, 0, 4096)
    set_wire(fake, c, KAFKA)
    assert run(fake, c, lines)[0] == 0  # (the ctx's buffers exist from here on)
    c0 = fake.fgf_calls()
    rc, out, n = run(fake, c, lines)
    calls = int(fake.fgf_calls() - c0)
    first = D.compressed(fake, c)
    assert rc == 0 and calls >= 25 and first["n_members"] >= 3
    bad = []
    for i in range(1, calls + 1):
        fake.fgf_fail_call_after(i)
        rc, _, _ = run(fake, c, lines)
        fake.fgf_fail_call_after(-1)
        why = []
        if rc != L.FG_ERR_HIP:
            why.append(f"rc {rc}")
        if abs(fake.fg_last_hip_error(c.h)) != fake.fgf_last_injected():
            why.append(f"fg_last_hip_error {fake.fg_last_hip_error(c.h)}, injected {fake.fgf_last_injected()}")
        if fake.fgf_in_flight() != 0:
            why.append(f"{fake.fgf_in_flight()} operations in flight")
        rc, out, n = run(fake, c, lines)
        again = D.compressed(fake, c)
        if rc != 0 or not np.array_equal(again["z"], first["z"]) or not np.array_equal(again["member_first"], first["member_first"]):
            why.append(f"the call after it: rc {rc} or another result")
        if why:
            bad.append((i, why))
    c.close()
    assert not bad, f"{len(bad)} of {calls} call indices: {bad}"


def test_sanitized_standalone_run_of_the_host_stages(tmp_path):
    """the scratch layouts, the member stage and the sized resident calls in a stand-alone program under AddressSanitizer and UBSan
    (tests/native/host_stages_san_main.cpp, on the fake runtime, whose device memory is malloc'd): the grid of the test above through the
    three transcode entries, the five resident entries at n = 0, 1, 63, 64, 65, 130 as a sizing call, at exact capacity and a byte
    short, a failed runtime call at every index of one kafka + gzip transcode.  Nothing loaded into Python is sanitized."""
    exe = tmp_path / "host_stages_san"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", "-Wno-unused-variable", "-fno-omit-frame-pointer",
           f"-I{H.HERE / 'fakehip'}", f"-I{H.ROOT / 'include'}", f"-I{D.CSRC}", f"-I{H.HERE}", str(H.HERE / "host_stages_san_main.cpp"), "-o", str(exe)]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    b = subprocess.run(cmd[:1] + san + cmd[1:], capture_output=True, text=True)
    if b.returncode != 0:
        # only a linker that cannot find the sanitizers' runtime may fall back to the plain build, which still runs every case, and
        # the run says so; anything else the sanitized build trips over is a failure
        assert "cannot find" in b.stderr and ("asan" in b.stderr or "ubsan" in b.stderr), b.stderr[-4000:]
        warnings.warn("no sanitizer runtime on this machine: host_stages_san_main.cpp ran WITHOUT AddressSanitizer / UBSan")
        subprocess.run(cmd, check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    # (AddressSanitizer says once on stderr that it does not fully support swapcontext -- the fibers of the wave emulation; an error ends the run)
    assert r.returncode == 0 and r.stdout.split() == ["ok", "48", "cells", "48", "resident", "45", "faults"] and "ERROR" not in r.stderr, r.stdout + r.stderr
