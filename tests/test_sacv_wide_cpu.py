"""CPU side of the wide SAC-v learner's tests: on the two oracles alone, every case of tests/_sacv_wide_cases.py keeps its state bars
at a tenth of the float64 oracle's movement or less — the condition under which the GPU comparison (tests/test_gpu_sacv_wide.py)
means something."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _state_parity as sp  # noqa: E402
from _sacv_wide_cases import CASES  # noqa: E402


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_sacv_wide_bars_are_a_tenth_of_the_movement_or_less(case):
    o64, _, o32, _ = sp.oracles(case)
    sp.compare_state(sp.oracle_exports(o32), o64, o32, sp.start_of(case), case.k)    # the float32 oracle itself is inside the bars
    ratio = sp.bar_over_movement(o64, o32, sp.start_of(case), case.k)
    bad = {k: v for k, v in ratio.items() if not v <= sp.MOVEMENT_SHARE}
    assert not bad, bad
