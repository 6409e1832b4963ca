"""CPU side of the wide SAC1 learner's tests: (1) on the two oracles alone, every case of tests/_sac1_wide_cases.py keeps its state bars
at a tenth of the float64 oracle's movement or less — the condition under which the GPU comparison (tests/test_gpu_sac1_wide.py) means
something; (2) the mode-3 learner layout (csrc/sac1_layout.h make_layout(..., wide); csrc/wide_pack.h w1wide_index), its segment
arithmetic restated in NumPy: external -> internal -> external is the identity and no pad is the image of an external index."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _state_parity as sp  # noqa: E402
from _sac1_wide_cases import CASES  # noqa: E402


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_wide_bars_are_a_tenth_of_the_movement_or_less(case):
    o64, _, o32, _ = sp.oracles(case)
    ratio = sp.bar_over_movement(o64, o32, sp.start_of(case), case.k)
    bad = {k: v for k, v in ratio.items() if not v <= sp.MOVEMENT_SHARE}
    assert not bad, bad


def _w1wide(d, j):   # column d (d = D: the bias) of hidden unit j: float4 d // 8 of lane half (d // 4) % 2, element d % 4
    return ((((j >> 5) * 4 + (d >> 3)) * 2 + ((d >> 2) & 1)) * 32 + (j & 31)) * 4 + (d & 3)


def _internal_index(o, a, h1, h2):
    """-> (internal index of every external element in external order, internal length)"""
    Kp1, Np2 = (h1 + 31) & ~31, (h2 + 31) & ~31
    idx, pos = [], 0
    pad4 = lambda n: (n + 3) & ~3  # noqa: E731
    for D, heads in ((o, (a, a)), (o + a, (1,)), (o + a, (1,))):   # pi, q1, q2
        pos = pad4(pos)
        d, j = np.meshgrid(np.arange(D + 1), np.arange(h1), indexing="ij")      # [W1 ; b1]: kernel rows, then the bias as column D
        idx.append(pos + _w1wide(d, j).reshape(-1))
        pos = pad4(pos + Kp1 * 32)
        k, j = np.meshgrid(np.arange(h1), np.arange(h2), indexing="ij")         # W2, k4-interleaved
        idx.append(pos + (((k >> 2) * Np2 + j) * 4 + (k & 3)).reshape(-1))
        pos += Kp1 * Np2
        idx.append(pos + np.arange(h2))
        pos += Np2
        for n in heads:                                                           # head kernel, then its bias padded to a float4
            idx.append(pos + np.arange(h2 * n + n))
            pos = pad4(pos + h2 * n + n)
    return np.concatenate(idx), pos


@pytest.mark.parametrize("o,a,h1,h2", [(27, 4, 72, 44), (24, 4, 400, 300)])
def test_wide_layout_round_trips(o, a, h1, h2):
    idx, total = _internal_index(o, a, h1, h2)
    n_ext = (o + 1) * h1 + 2 * (o + a + 1) * h1 + 3 * (h1 + 1) * h2 + 2 * (h2 + 1) * a + 2 * (h2 + 1)
    assert idx.size == n_ext and idx.min() >= 0 and idx.max() < total and np.unique(idx).size == n_ext   # one slot each: pads are nobody's image
    ext = np.arange(1, n_ext + 1, dtype=np.float32)
    internal = np.zeros(total, np.float32)
    internal[idx] = ext
    assert np.array_equal(internal[idx], ext) and np.count_nonzero(internal) == n_ext                       # ... and the rest stays zero
    d = np.arange(o + a + 1)
    assert np.array_equal(_w1wide(d, 0) // 4 % 64 // 32, (d // 4) % 2) and np.array_equal(_w1wide(d, 0) // 256, d // 8) and np.array_equal(_w1wide(d, 0) % 4, d % 4)
