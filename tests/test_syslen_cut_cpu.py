"""CPU: the per-segment cut of fg_transcode_multi_batch (flowgger_amd/csrc/fg_syslen_multi.hpp: cut_find / cut_mark) on the wave
emulation, against its five-line model: behind the first payload of a segment that is not UTF-8 every frame of that segment becomes
FG_SLOT_UNREACHED, and nothing else changes."""
import numpy as np
import pytest

from syslen_cut_binding import SyslenCutHost
from transcode_multi_model import UNREACHED, cut, cut_hazards, random_cases


@pytest.fixture(scope="module")
def host():
    return SyslenCutHost()


def test_the_mark_is_the_slot_kind(host):
    from flowgger_amd import _lib as L

    assert host.mark == UNREACHED == L.FG_SLOT_UNREACHED == 3


@pytest.mark.parametrize("name,first,bad", cut_hazards(), ids=[c[0] for c in cut_hazards()])
@pytest.mark.parametrize("reverse", [False, True], ids=["groups in order", "groups reversed"])
def test_the_hazard_list(host, name, first, bad, reverse):
    want = cut(bad, first)
    got = host.cut(np.asarray(bad, np.uint8), first, reverse)
    assert got.tolist() == want
    if sum(bad) and name.startswith(("two flagged", "3000 frames")):
        assert UNREACHED in want and want.count(1) == 1


def test_the_model_on_the_case_a_chain_of_stages_gets_wrong():
    assert cut([0, 1, 0, 0, 0, 1, 1], [0, 4, 5, 7]) == [0, 1, UNREACHED, UNREACHED, 0, 1, UNREACHED]


def test_a_seeded_sweep_of_random_segments_and_verdicts(host):
    cases = flagged = empties = 0
    for first, bad in random_cases(seed=20, count=300):
        want = cut(bad, first)
        assert host.cut(np.asarray(bad, np.uint8), first, bool(cases & 1)).tolist() == want, (first, bad)
        cases += 1
        flagged += UNREACHED in want
        empties += any(a == b == c for a, b, c in zip(first, first[1:], first[2:]))
    assert cases == 300 and flagged > 50 and empties > 50
