"""CPU: the two forms of the framers' UTF-8 rule against each other and against Python's decoder.  The scalar form
(flowgger_amd/csrc/fg_utf8.hpp: err_at, cut_off, payload_bad) judges payloads for the octet-counted framers, the UDP unpacker, the
host hops and the boundary patches of the segmented framer; the dword-parallel form (fg_fuse.hpp: utf8_err_flags inside chunk_masks)
is what every line / NUL framing kernel runs, and the segmented framer patches bits of the first into mask words of the second -- they
must agree bit for bit.  Every byte of the alphabet below is an edge of a class the rule tells apart (ASCII, the continuation ranges
80..8F / 90..9F / A0..BF, the leads C0 C1 | C2..DF | E0 | E1..EC | ED | EE EF | F0 | F1..F3 | F4 | F5..FF), and the rule at a position
looks at four bytes: all 24^4 four-byte strings are every combination of classes it can see."""
from __future__ import annotations

import itertools

import numpy as np
import pytest

from fuse_binding import FuseHost

ALPHABET = bytes.fromhex("007F808F909FA0BFC0C1C2DFE0E1ECEDEEEFF0F1F3F4F5FF")
REMS = [-1, 0, 1, 3, 4, 5, 15, 16]


@pytest.fixture(scope="module")
def host():
    return FuseHost()


def test_alphabet():
    assert len(ALPHABET) == 24 and len(set(ALPHABET)) == 24


def test_scalar_rule_equals_python_decoder(host):
    """(a) the scalar rule flags some position 0 .. 4 of a string (the bytes before it read as 0, position 4 with b = 0) <=>
    bytes.decode('utf-8') raises; all 331 776 strings"""
    got = host.scalar_bad4(ALPHABET)

    def raises(s: bytes) -> int:
        try:
            s.decode("utf-8")
            return 0
        except UnicodeDecodeError:
            return 1

    want = np.fromiter((raises(bytes(t)) for t in itertools.product(ALPHABET, repeat=4)), np.uint8, len(ALPHABET) ** 4)
    diff = np.flatnonzero(got != want)
    assert 0 < int(want.sum()) < want.size  # (both verdicts occur)
    assert diff.size == 0, f"{diff.size} strings differ, the first: {bytes(list(itertools.product(ALPHABET, repeat=4))[int(diff[0])]).hex()}"


@pytest.mark.parametrize("delim", [0x0A, 0x00])
def test_dword_rule_equals_scalar_rule(host, delim):
    """(b) + (c): chunk_masks' error half == the scalar rule and its delimiter half == a byte compare, position by position, for every
    string at every byte offset of a dword and every rem (fgf_rule_sweep, tests/native/fuse_host.cpp, says how the chunks are laid out)"""
    wrong, first, (triples, err_bits, delim_bits) = host.rule_sweep(ALPHABET, REMS, delim)
    assert triples == 24 ** 4 * 4 * len(REMS)
    assert err_bits > 0 and (delim_bits > 0) == (delim in ALPHABET)  # (the sweep saw what it is about)
    i, o, rem, got, want = first
    assert wrong == 0, (f"{wrong} of {triples} words differ; the first: string {bytes(list(itertools.product(ALPHABET, repeat=4))[i]).hex()} phase {o} rem {rem}: "
                        f"chunk_masks {got:#010x}, scalar rule {want:#010x}")


def test_delimiter_half_on_delimiter_bytes(host):
    """(c) once more over bytes that ARE delimiters or differ from one in a single bit (0A never occurs in the alphabet above)"""
    alphabet = bytes.fromhex("000A0B8A80FF")
    for delim in (0x0A, 0x00):
        wrong, first, (triples, _, delim_bits) = host.rule_sweep(alphabet, REMS, delim)
        assert triples == 6 ** 4 * 4 * len(REMS) and delim_bits > 0
        assert wrong == 0, (delim, first)


def test_chunk_masks_by_hand(host):
    """single chunks through the plain export, worked out by hand: the bit AT rem is the cut-off verdict, nothing lies behind it"""
    chunk = bytes.fromhex("E282AC0A") + b"abc\n" + bytes.fromhex("F09F9880") + b"\n\n\0\xC3"
    assert host.chunk_masks(chunk, b"abcd", 0x0A, 16) == 0x3088
    assert host.chunk_masks(chunk, b"abc\xC3", 0x0A, 16) == 0x3088 | 1 << 16  # (a lead in front of the chunk: E2 is not its continuation)
    assert host.chunk_masks(chunk, b"abcd", 0x0A, 2) == 1 << 18  # (E2 82 cut off at position 2)
    assert host.chunk_masks(chunk, b"abcd", 0x0A, 3) == 0
    assert host.chunk_masks(chunk, b"abcd", 0x0A, 15) == 0x3088  # (the C3 behind the end reads as 0)
    assert host.chunk_masks(chunk, b"abcd", 0x0A, -1) == 0
    assert host.chunk_masks(chunk, b"abcd", 0x00, 16) == 0x4000  # (the lead C3 is no error where it stands: the NEXT chunk's first byte is judged against it)
