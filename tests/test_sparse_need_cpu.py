"""CPU: the need-range arithmetic of the sparse RFC5424 window (flowgger_amd/csrc/fg_sparse_need.hpp) against a byte-by-byte model.

The kernel leaves a 16-byte chunk of a group's window unfetched unless it overlaps the first H bytes or the last bytes of a line of
the group.  tests/native/sparse_need_host.cpp marks chunks with the header's functions the way the kernel does -- one run per line,
one more for the last line's end -- and compares with the model for every alignment of the first line, every line length around H,
runs of empty and one-byte lines, and random groups: every byte of every head and of every line's end lies in a marked chunk, and no
chunk is marked that overlaps neither."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_marked_chunks_are_exactly_the_model_s(tmp_path):
    exe = tmp_path / "sparse_need_host"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", str(ROOT / "tests/native/sparse_need_host.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    assert r.stdout.strip().endswith(" 0 errors"), r.stdout
