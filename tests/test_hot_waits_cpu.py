"""CPU (needs hipcc, no GPU): the memory waits of the RFC5424 headline kernel's group loop, read off its device assembly.

gfx950 counts loads and stores on one counter, vmcnt, and retires them in order.  Inside the streaming loop (fg_pipeline.hpp
persistent_loop) a wait that names vmcnt, anywhere between the first row store and the end of stage B's straight-line fast path, is a
wait for the ten row stores or for the next group's whole register window: the overlap the window exists for is gone.  tools/hot_waits.py
lists those waits by the FG_MARK() they follow; this test holds the list empty where it has to be.  It looks at waits, nothing else."""
import json
import shutil
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else None)

pytestmark = pytest.mark.skipif(HIPCC is None, reason="needs hipcc (cross-compiles for gfx950; no GPU needed)")

HEADLINE = "k_rfc5424ILi20ELb0ELb0ELb0E"  # fg::k_rfc5424<20, false, false, false>: whole short lines, no pair-parallel walk


@pytest.fixture(scope="module")
def headline():
    """one compile of fg_rfc5424.hip (about a minute), shared by the tests below"""
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "hot_waits.py"), str(ROOT / "flowgger_amd" / "csrc" / "fg_rfc5424.hip"), HEADLINE,
                        "--json"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout)


def test_the_marks_are_there_and_in_order(headline):
    """the listing is by position in the text: the loop's marks once each and in the loop's order, every rare bracket paired"""
    order = [m["mark"] for m in headline["marks"] if m["mark"] not in ("RARE_BEGIN", "RARE_END")]
    assert order == ["A", "S", "ST", "W0", "W1", "B", "F", "Z"], order
    assert not headline["warnings"], headline["warnings"]


def test_no_wait_between_the_first_row_store_and_the_last_window_load(headline):
    """ST stands in front of the first row store, W1 behind the last window load"""
    bad = [w for w in headline["waits"] if w["after"] in ("ST", "W0")]
    assert not bad, bad


def test_no_wait_on_the_fast_path_behind_the_prefetch(headline):
    """W1 / B .. F: the terminator strip and the straight-line header parse.  Only a bracketed rare block (the line longer than the
    tile, whose last bytes come from global memory) may wait."""
    bad = [w for w in headline["waits"] if w["after"] in ("W1", "B") and not w["rare"]]
    assert not bad, bad
    assert any(w["after"] in ("W1", "B") and w["rare"] for w in headline["waits"]), "the oversize line's block waits for its own loads"


def test_registers(headline):
    assert headline["vgprs"] is not None and headline["vgprs"] <= 209, headline["vgprs"]
    assert headline["scratch"] == 0, headline["scratch"]
