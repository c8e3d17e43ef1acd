"""The UDP input's inflate core (flowgger_amd/csrc/fg_inflate.hpp) compiled for the CPU, datagram by datagram, against the model of
handle_record_maybe_compressed with Python's zlib as the inflater (tests/udp_model.py).  Exact on verdict and bytes."""
import zlib

import numpy as np
import pytest

import udp_model as um


@pytest.fixture(scope="module")
def host():
    return um.InflateHost()


def _run(host, datagrams, max_inflated=um.DEFAULT_MAX, what=""):
    offs, packed, drop, status = host.unpack(datagrams, max_inflated)
    um.check_batch(datagrams, max_inflated, offs, packed, drop, status, what)
    return status


def test_reference_vectors(host):
    cases = dict(um.case_list())
    st = _run(host, [cases["ref_raw"], cases["ref_zlib"], cases["ref_gzip"], cases["ref_gzip_trunc5"]])
    assert list(st) == [um.RAW, um.ZLIB, um.GZIP, um.BAD_UTF8]
    assert um.ERRORS[um.BAD_UTF8] == um.VECTORS["bad_record_error"]
    offs, packed, _, _ = host.unpack([cases["ref_zlib"], cases["ref_gzip"]])
    assert bytes(packed[:offs[1]]) == um.REF_LINE and bytes(packed[offs[1]:offs[2]]) == um.REF_LINE


def test_case_list(host):
    cases = um.case_list()
    st = dict(zip([n for n, _ in cases], _run(host, [d for _, d in cases])))
    # the model's answers are what the issue says they are
    for name, want in (("stored", um.ZLIB), ("fixed", um.ZLIB), ("dynamic", um.ZLIB), ("flush_sync", um.ZLIB), ("flush_full", um.ZLIB),
                       ("stored_two_blocks", um.ZLIB), ("dist1_overlap", um.ZLIB), ("dist32768", um.ZLIB), ("match_at_cap", um.ZLIB),
                       ("match_past_cap", um.TOO_LARGE), ("match_at_cap_gz", um.GZIP), ("match_past_cap_gz", um.TOO_LARGE),
                       ("zlib_len7", um.BAD_UTF8), ("gzip_len23", um.BAD_UTF8), ("second_byte_5e", um.BAD_UTF8), ("empty", um.RAW),
                       ("gz_fextra", um.GZIP), ("gz_fname", um.GZIP), ("gz_fcomment", um.GZIP), ("gz_fhcrc", um.GZIP), ("gz_all4", um.GZIP),
                       ("gz_bad_fhcrc", um.BAD_GZIP), ("gz_bad_crc32", um.BAD_GZIP), ("gz_bad_isize", um.BAD_GZIP),
                       ("zlib_bad_adler", um.BAD_ZLIB), ("zlib_trailing", um.ZLIB), ("gzip_trailing", um.GZIP),
                       ("zlib_bad_utf8", um.BAD_UTF8), ("gzip_cut_utf8", um.BAD_UTF8), ("gz_reserved_flag", um.BAD_GZIP)):
        assert st[name] == want, name


def test_block_types_are_what_they_claim():
    cases = dict(um.case_list())
    btype = lambda z: (z[2] >> 1) & 3
    assert btype(cases["stored"]) == 0 and btype(cases["fixed"]) == 1 and btype(cases["dynamic"]) == 2
    assert cases["flush_sync"].count(b"\x00\x00\xff\xff") >= 2  # the empty stored blocks


@pytest.mark.parametrize("cap", [1, 2, 258, 259, 1000, 4096])
def test_small_caps(host, cap):
    """the cap inside literals, matches and stored blocks"""
    ds = [zlib.compress(b"q" * k, lvl) for k in (cap - 1, cap, cap + 1, cap + 2, cap + 300) for lvl in (0, 6)]
    ds += [um.gz_member(bytes(range(32, 120)) * 40, level=lvl)[:] for lvl in (0, 1, 9)]
    _run(host, ds, cap, f"cap {cap}")


def test_every_truncation(host):
    _run(host, um.truncations(), what="truncations")


def test_mutation_fuzz(host):
    pool = um.mutation_pool()
    assert len(pool) == 20_000
    # (um.model lets anything but zlib.error through: the model itself never raises anything else on this pool)
    st = _run(host, pool, what="mutation pool")
    counts = np.bincount(st, minlength=7)
    assert counts[um.BAD_ZLIB] > 1000 and counts[um.BAD_GZIP] > 1000 and counts[um.BAD_UTF8] > 100 and counts[um.ZLIB] + counts[um.GZIP] > 0, counts


def test_mutation_fuzz_small_cap(host):
    """the same pool under a cap most lines exceed: TOO_LARGE against zlib's max_length"""
    pool = um.mutation_pool(4000, seed=7)
    st = _run(host, pool, 200, "mutation pool, cap 200")
    assert np.bincount(st, minlength=7)[um.TOO_LARGE] > 100


def test_hand_table_is_what_zlib_says():
    """every hand-built stream reaches the inflater and gets the verdict its table expects from Python's zlib: a case that stopped
    reaching it (the gate, the padding, a slip in the bit writer) fails here instead of passing vacuously everywhere else"""
    for cap in um.HAND_CAPS:
        table = um.hand_streams(cap)
        assert len({n for n, _, _ in table}) == len(table) >= 140
        for name, d, want in table:
            assert um.gate(d) == {"z": um.ZLIB, "g": um.GZIP}[name.replace("_check_off_by_one", "")[-1]], name
            if name.startswith("cap_") or cap == um.DEFAULT_MAX:
                assert um.model(d, cap)[0] == want, f"{name} at cap {cap}: zlib says {um.model(d, cap)[0]}, the table {want}"
    # what the orderings at the cap rest on: a complete stream of cap + 1 bytes keeps its bytes, the others none
    for name, d, _ in um.hand_streams(257):
        if name.startswith("cap_"):
            assert len(um.model(d, 257)[1]) == (258 if "_then_eob_" in name and "off_by_one" not in name else 0), name


@pytest.mark.parametrize("cap", um.HAND_CAPS)
def test_hand_streams(host, cap):
    table = um.hand_streams(cap)
    st = _run(host, [d for _, d, _ in table], cap, f"hand-built streams, cap {cap}")
    for (name, _, want), got in zip(table, st):
        if name.startswith("cap_") or cap == um.DEFAULT_MAX:
            assert got == want, name


def test_random_code_sets(host):
    good, flipped = um.random_code_set_pool()
    assert len(good) == len(flipped) == 2000
    st_good, _, _ = um.expect(good)
    st_flip, _, _ = um.expect(flipped)
    # conditions on the generator, from the model's answers: every stream is valid, and a flipped header bit mostly is not
    assert bool(((st_good == um.ZLIB) | (st_good == um.GZIP)).all()), np.bincount(st_good, minlength=7)
    assert int(((st_flip == um.BAD_ZLIB) | (st_flip == um.BAD_GZIP)).sum()) >= len(flipped) // 2, np.bincount(st_flip, minlength=7)
    _run(host, good + flipped, what="random code sets")
    _run(host, good[:400] + flipped[:400], 200, "random code sets, cap 200")


def test_sanitized_standalone_run(tmp_path):
    """fg_inflate.hpp in a stand-alone program under AddressSanitizer and UBSan, over the hand-built streams at every cap and the
    random code sets: malformed headers are where a table index would run off.  The program checks nothing but its own sanity;
    what the answers must be is the other tests' business."""
    import struct
    import subprocess
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    exe = tmp_path / "inflate_sanitized"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    f"-I{root / 'flowgger_amd' / 'csrc'}", str(root / "tests/native/inflate_host.cpp"), str(root / "tests/native/inflate_sanitized_main.cpp"),
                    "-o", str(exe)], check=True)
    good, flipped = um.random_code_set_pool()
    for k, cap in enumerate(um.HAND_CAPS):
        grams = [d for _, d, _ in um.hand_streams(cap)] + (good + flipped if k == 0 else flipped[:300])
        f = tmp_path / f"grams_{cap}.bin"
        f.write_bytes(b"".join(struct.pack("<I", len(g)) + g for g in grams))
        r = subprocess.run([str(exe), str(f), str(cap)], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "" and r.stdout.split()[:2] == ["OK", str(len(grams))], r.stdout + r.stderr
        # (the same library code as InflateHost: the two builds give the same total)
        assert int(r.stdout.split()[2]) == sum(len(s) for s in um.expect(grams, cap)[2])


def test_udp_batcher_keeps_its_state_when_a_flush_fails(tmp_path):
    """fg::UdpBatcher against a library whose fg_udp_decode_batch fails (the fake launchers have no inflate kernels:
    FG_ERR_UNSUPPORTED): the datagrams stay parked as they were, without the 16 bytes of slack, and later ones line up behind them"""
    import subprocess
    from pathlib import Path

    import test_host_pipeline_cpu as hp

    if not hp.LIB.exists() or any(s.stat().st_mtime > hp.LIB.stat().st_mtime for s in hp.SRC):  # (as that module's fixture builds it)
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                        "-Wno-unused-variable", f"-I{hp.HERE / 'fakehip'}", f"-I{hp.ROOT / 'include'}", "-o", str(hp.LIB),
                        str(hp.HERE / "host_pipeline_fake.cpp")], check=True)
    root = Path(__file__).resolve().parent.parent
    exe = tmp_path / "udp_batcher_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", str(root / "tests/native/udp_batcher_test.cpp"), "-o", str(exe), f"-I{root / 'include'}",
                    f"-I{root / 'flowgger_amd/host'}", str(hp.LIB), f"-Wl,-rpath,{hp.HERE}"], check=True)
    r = subprocess.run([str(exe), "fail"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "OK", r.stdout + r.stderr
