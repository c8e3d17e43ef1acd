"""CPU (needs hipcc, no GPU): the memory waits of the sparse-window RFC5424 kernel's group loop, read off its device assembly.

The same listing as tests/test_hot_waits_cpu.py (tools/hot_waits.py), for fg::k_rfc5424_sparse<20, false, 96>.  The sparse window builds
its need bitmap in LDS between the next group's geometry and the row stores and gives every load its offset in a register; none of that
may put a wait that names vmcnt behind the first row store: it would be a wait for the row stores or for the whole next window.

Registers, as compiled when this test was written: 235 VGPRs, no scratch (the whole-line kernel takes 208; the head form carries the
whole-line decode a second time, coop_redo).  The bound is what two waves per SIMD allow, which the launch needs (eight waves per CU)."""
import json
import shutil
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else None)

pytestmark = pytest.mark.skipif(HIPCC is None, reason="needs hipcc (cross-compiles for gfx950; no GPU needed)")

SPARSE = "k_rfc5424_sparseILi20ELb0ELj96E"  # fg::k_rfc5424_sparse<20, false, 96>


@pytest.fixture(scope="module")
def sparse():
    """one compile of fg_rfc5424.hip (about a minute), shared by the tests below"""
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "hot_waits.py"), str(ROOT / "flowgger_amd" / "csrc" / "fg_rfc5424.hip"), SPARSE,
                        "--json"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout)


def test_the_marks_are_there_and_in_order(sparse):
    """the loop's marks once each and in the loop's order (the whole-line decode inside coop_redo carries none), every rare bracket paired"""
    order = [m["mark"] for m in sparse["marks"] if m["mark"] not in ("RARE_BEGIN", "RARE_END")]
    assert order == ["A", "S", "ST", "W0", "W1", "B", "F", "Z"], order
    assert not sparse["warnings"], sparse["warnings"]


def test_no_wait_between_the_first_row_store_and_the_last_window_load(sparse):
    bad = [w for w in sparse["waits"] if w["after"] in ("ST", "W0")]
    assert not bad, bad


def test_no_wait_on_the_fast_path_behind_the_prefetch(sparse):
    """W1 / B .. F: the strip, the last byte out of the tile, the straight-line header parse; only a bracketed rare block may wait"""
    bad = [w for w in sparse["waits"] if w["after"] in ("W1", "B") and not w["rare"]]
    assert not bad, bad


def test_registers(sparse):
    print("NumVgprs", sparse["vgprs"], "ScratchSize", sparse["scratch"])
    assert sparse["vgprs"] is not None and sparse["vgprs"] <= 256, sparse["vgprs"]
    assert sparse["scratch"] == 0, sparse["scratch"]
