"""CPU: fg_set_deflate_mode through the host side (fg_capi.cpp: fg_deflate_front and its callers) on the fake runtime of
test_deflate_host_cpu.py plus the block launcher of FG_DEFLATE_DYNAMIC (tests/native/host_pipeline_fake_deflate_dyn.cpp); with that
file's own library, which lacks the launcher, the build-without-the-kernel answer."""
import ctypes as C
import subprocess
import zlib

import numpy as np
import pytest

import deflate_dyn_model as ddm
import deflate_model as dm
import test_deflate_host_cpu as T
import test_host_pipeline_cpu as H
from flowgger_amd import _lib as L
from test_host_pipeline_cpu import Ctx

u64, vp = C.c_uint64, C.c_void_p
LIB = H.HERE / "libhost_pipeline_fake_deflate_dyn.so"
SRC = [H.HERE / "host_pipeline_fake_deflate_dyn.cpp", H.HERE / "deflate_dyn_driver.hpp"] + T.SRC


def load(path, srcs):
    """build (when stale) and open a fake library, with the prototypes test_deflate_host_cpu.py's fixture sets and this file's own"""
    if not path.exists() or any(s.stat().st_mtime > path.stat().st_mtime for s in srcs):
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                        "-Wno-unused-variable", f"-I{H.HERE / 'fakehip'}", f"-I{H.ROOT / 'include'}", f"-I{T.CSRC}", f"-I{H.HERE}", "-o", str(path), str(srcs[0])],
                       check=True)
    lib = C.CDLL(str(path))
    lib.fg_create.argtypes = [C.c_int, vp, C.POINTER(vp)]
    lib.fg_destroy.argtypes = [vp]
    lib.fg_destroy.restype = None
    lib.fg_clone.argtypes = [vp, C.POINTER(vp)]
    lib.fg_last_hip_error.argtypes = [vp]
    lib.fg_transcode_batch.argtypes = [vp, C.c_int, C.c_int, C.POINTER(L.fg_encode_cfg), vp, u64, vp, u64, C.c_int, C.POINTER(L.fg_transcoded)]
    lib.fg_transcode_multi_batch.argtypes = [vp, C.c_int, C.c_int, C.POINTER(L.fg_encode_cfg), vp, u64, vp, vp, u64, C.POINTER(L.fg_transcoded_multi)]
    lib.fg_udp_transcode_batch.argtypes = [vp, C.c_int, C.POINTER(L.fg_encode_cfg), vp, u64, vp, u64, u64, C.POINTER(L.fg_transcoded), C.POINTER(vp)]
    lib.fg_set_output_compression.argtypes = [vp, C.POINTER(L.fg_compress_cfg)]
    lib.fg_set_deflate_mode.argtypes = [vp, C.c_int]
    lib.fg_last_compressed.argtypes = [vp, C.POINTER(L.fg_compressed)]
    lib.fg_deflate_device.argtypes = [vp, vp, u64, vp, u64, vp, u64, vp, C.POINTER(u64), vp]
    lib.fg_deflate_block_bytes.restype = C.c_uint32
    lib.fgf_fail_call_after.argtypes = [C.c_longlong]
    lib.fgf_calls.restype = lib.fgf_in_flight.restype = C.c_ulonglong
    return lib


@pytest.fixture(scope="module")
def lib():
    lib = load(LIB, SRC)
    lib.fgf_deflate_dyn_launches.restype = C.c_ulonglong
    lib.fgf_deflate_mode.argtypes = [vp]
    return lib


@pytest.fixture(scope="module")
def old():
    """the library of test_deflate_host_cpu.py: every launcher but fg_launch_deflate_blocks_dyn"""
    return load(T.LIB, T.SRC)


def set_mode(lib, c, mode):
    assert lib.fg_set_deflate_mode(c.h, mode) == 0


def test_argument_errors_and_the_default(lib):
    c = Ctx(lib)
    assert lib.fgf_deflate_mode(c.h) == L.FG_DEFLATE_FIXED == 0 and L.FG_DEFLATE_DYNAMIC == 1
    assert lib.fg_set_deflate_mode(None, L.FG_DEFLATE_DYNAMIC) == L.FG_ERR_ARG
    for bad in (2, -1, 7):
        assert lib.fg_set_deflate_mode(c.h, bad) == L.FG_ERR_ARG and lib.fgf_deflate_mode(c.h) == L.FG_DEFLATE_FIXED
    set_mode(lib, c, L.FG_DEFLATE_DYNAMIC)
    assert lib.fg_set_deflate_mode(c.h, 2) == L.FG_ERR_ARG and lib.fgf_deflate_mode(c.h) == L.FG_DEFLATE_DYNAMIC
    c.close()


def deflate_device(lib, c, members, cap=None, out=None):
    blob, cuts = dm.pack_members(members)
    n = len(members)
    zoff, total = np.zeros(n + 1, np.uint64), u64()
    rc = lib.fg_deflate_device(c.h, blob.ctypes.data, int(cuts[-1]), cuts.ctypes.data, n, None if out is None else out.ctypes.data,
                               0 if cap is None else cap, zoff.ctypes.data, C.byref(total), vp(-1))
    return rc, int(total.value), zoff


MEMBERS = [b"k=v " * 100, b"", bytes(range(256)) * 3, dm.equal_members(1)[0] * 30]


def test_fixed_named_or_not_is_what_it_was(lib, old):
    """the default, FG_DEFLATE_FIXED named, and fixed again after dynamic: the parent's bytes, the fixed launcher once, the new one never"""
    want = None
    for which, how in ((old, "parent"), (lib, "default"), (lib, "named"), (lib, "after_dynamic")):
        c = Ctx(which)
        if how == "after_dynamic":
            set_mode(which, c, L.FG_DEFLATE_DYNAMIC)
        if how in ("named", "after_dynamic"):
            set_mode(which, c, L.FG_DEFLATE_FIXED)
        T.launches(which)
        lib.fgf_deflate_dyn_launches(1)
        rc, need, _ = deflate_device(which, c, MEMBERS)
        out = np.full(need + 8, 0xEE, np.uint8)
        rc2, _, zoff = deflate_device(which, c, MEMBERS, need, out)
        assert rc == 0 and rc2 == 0 and which.fgf_in_flight() == 0
        assert T.launches(which) == [0, 2, 2, 2, 1] and lib.fgf_deflate_dyn_launches(1) == 0, how
        got = (out.tobytes(), zoff.tolist())
        want = want or got
        assert got == want, how
        c.close()
    for entry in sorted(T.ENTRIES):
        lines, seen = T.lines_of(300), []
        for how in ("default", "named"):
            c = Ctx(lib)
            T.set_compression(lib, c, L.FG_COMP_GZIP, 0, 4096)
            if how == "named":
                set_mode(lib, c, L.FG_DEFLATE_FIXED)
            assert T.ENTRIES[entry](lib, c, lines)[0] == 0
            T.launches(lib)
            c0 = lib.fgf_calls()
            assert T.ENTRIES[entry](lib, c, lines)[0] == 0 and lib.fgf_in_flight() == 0
            z = T.compressed(lib, c)
            seen.append((z["z"].tobytes(), z["z_offsets"].tolist(), int(lib.fgf_calls() - c0), T.launches(lib), int(lib.fgf_deflate_dyn_launches(1))))
            c.close()
        assert seen[0] == seen[1] and seen[0][3] == [1] * 5 and seen[0][4] == 0, entry


def test_dynamic_through_fg_deflate_device(lib):
    B = int(lib.fg_deflate_block_bytes())
    c = Ctx(lib)
    set_mode(lib, c, L.FG_DEFLATE_DYNAMIC)
    T.launches(lib)
    lib.fgf_deflate_dyn_launches(1)
    rc, need, sized = deflate_device(lib, c, MEMBERS)  # the sizing call
    assert rc == 0 and lib.fgf_in_flight() == 0 and int(sized[-1]) == need
    assert T.launches(lib) == [0, 1, 0, 1, 0] and lib.fgf_deflate_dyn_launches(1) == 1
    out = np.full(need + 8, 0xEE, np.uint8)
    rc, total, _ = deflate_device(lib, c, MEMBERS, need - 1, out)
    assert rc == L.FG_ERR_ENT_OVERFLOW and total == need and (out == 0xEE).all() and lib.fgf_in_flight() == 0
    rc, total, zoff = deflate_device(lib, c, MEMBERS, need, out)  # the exact fit
    assert rc == 0 and total == need and (out[need:] == 0xEE).all() and np.array_equal(zoff, sized) and lib.fgf_in_flight() == 0
    dm.check_members(MEMBERS, out[:need], zoff, B, "fg_deflate_device, dynamic")
    host = ddm.DynHost()
    assert dm.split(out[:need], zoff) == ddm.emulate(host, MEMBERS, ddm.DYNAMIC, workers=2)
    assert ddm.btype(dm.split(out[:need], zoff)[0]) == 2  # (a period of four: three symbols and a distance)
    set_mode(lib, c, L.FG_DEFLATE_FIXED)
    rc, fixed_need, _ = deflate_device(lib, c, MEMBERS)
    assert rc == 0 and need < fixed_need
    c.close()


@pytest.mark.parametrize("entry", sorted(T.ENTRIES))
def test_dynamic_through_the_transcode_calls(lib, entry):
    B = int(lib.fg_deflate_block_bytes())
    lines = T.lines_of(300)
    c = Ctx(lib)
    rc, out, n = T.ENTRIES[entry](lib, c, lines)
    assert rc == 0
    plain = T.result(out, n)
    T.set_compression(lib, c, L.FG_COMP_GZIP, 0, 4096)
    assert T.ENTRIES[entry](lib, c, lines)[0] == 0
    fixed = T.compressed(lib, c)
    set_mode(lib, c, L.FG_DEFLATE_DYNAMIC)
    T.launches(lib)
    lib.fgf_deflate_dyn_launches(1)
    rc, out, n2 = T.ENTRIES[entry](lib, c, lines)
    assert rc == 0 and lib.fgf_in_flight() == 0 and n2 == n
    assert T.launches(lib) == [1, 1, 0, 1, 1] and lib.fgf_deflate_dyn_launches(1) == 1
    got = T.result(out, n)
    assert got["out"] is None and got["out_bytes"] == len(plain["out"])
    for k in ("out_offsets", "meta", "enc_status"):
        assert np.array_equal(got[k], plain[k]), k
    z = T.compressed(lib, c)
    first, cuts = dm.model_members(plain["out_offsets"], 0, 4096, B)
    assert np.array_equal(z["member_first"], first) and np.array_equal(z["member_first"], fixed["member_first"]) and z["raw_bytes"] == len(plain["out"])
    raw = [plain["out"][int(cuts[k]):int(cuts[k + 1])] for k in range(len(cuts) - 1)]
    dm.check_members(raw, z["z"], z["z_offsets"], B, entry)
    assert b"".join(zlib.decompress(m, 31) for m in dm.split(z["z"], z["z_offsets"]) if m) == plain["out"]
    assert z["z"].size < fixed["z"].size and any(ddm.btype(m) == 2 for m in dm.split(z["z"], z["z_offsets"]) if m)
    # the mode survives fg_clone, as the compression cfg does
    h2 = vp()
    assert lib.fg_clone(c.h, C.byref(h2)) == 0 and lib.fgf_deflate_mode(h2) == L.FG_DEFLATE_DYNAMIC
    lib.fg_destroy(h2)
    # ... and back to no compression on the same ctx: the mode alone compresses nothing
    T.set_compression(lib, c, L.FG_COMP_NONE)
    T.launches(lib)
    rc, out, n = T.ENTRIES[entry](lib, c, lines)
    assert rc == 0 and T.result(out, n)["out"] == plain["out"] and T.compressed(lib, c)["n_members"] == 0
    assert T.launches(lib) == [0] * 5 and lib.fgf_deflate_dyn_launches(1) == 0
    c.close()


def test_a_build_without_the_dynamic_launcher(old):
    """the existing fake library: every launcher but the new one.  Dynamic mode answers FG_ERR_UNSUPPORTED from the calls that would
    compress, leaves nothing in flight, and the ctx goes on in fixed mode"""
    c = Ctx(old)
    set_mode(old, c, L.FG_DEFLATE_DYNAMIC)
    rc, total, _ = deflate_device(old, c, MEMBERS)
    assert rc == L.FG_ERR_UNSUPPORTED and total == 0 and old.fgf_in_flight() == 0
    lines = T.lines_of(120)
    for entry in sorted(T.ENTRIES):
        assert T.ENTRIES[entry](old, c, lines)[0] == 0  # (no compression set: nothing to refuse)
    T.set_compression(old, c, L.FG_COMP_GZIP, 7)
    for entry in sorted(T.ENTRIES):
        assert T.ENTRIES[entry](old, c, lines)[0] == L.FG_ERR_UNSUPPORTED and old.fgf_in_flight() == 0, entry
    set_mode(old, c, L.FG_DEFLATE_FIXED)
    for entry in sorted(T.ENTRIES):
        assert T.ENTRIES[entry](old, c, lines)[0] == 0 and T.compressed(old, c)["n_members"] > 0 and old.fgf_in_flight() == 0, entry
    c.close()


@pytest.mark.parametrize("entry", sorted(T.ENTRIES))
def test_a_failed_runtime_call_at_every_index_in_dynamic_mode(lib, entry):
    lines = T.lines_of(120)
    c = Ctx(lib)
    T.set_compression(lib, c, L.FG_COMP_GZIP, 0, 4096)
    set_mode(lib, c, L.FG_DEFLATE_DYNAMIC)
    assert T.ENTRIES[entry](lib, c, lines)[0] == 0
    c0 = lib.fgf_calls()
    rc, out, n = T.ENTRIES[entry](lib, c, lines)
    calls = int(lib.fgf_calls() - c0)
    first = T.compressed(lib, c)
    assert rc == 0 and calls >= 25 and first["n_members"] >= 3
    bad = []
    for i in range(1, calls + 1):
        lib.fgf_fail_call_after(i)
        rc, _, _ = T.ENTRIES[entry](lib, c, lines)
        lib.fgf_fail_call_after(-1)
        if rc != L.FG_ERR_HIP or lib.fgf_in_flight() != 0:
            bad.append((i, rc, int(lib.fgf_in_flight())))
    rc, out, n = T.ENTRIES[entry](lib, c, lines)
    assert rc == 0 and np.array_equal(T.compressed(lib, c)["z"], first["z"]) and lib.fgf_in_flight() == 0
    c.close()
    assert not bad, bad
