"""CPU side of the direct-operand DQN / SQN learner's tests, on the two oracles alone: (1) every case of tests/_dqn_direct_cases.py keeps
its whole-vector state bars at a tenth of the float64 oracle's movement or less — the condition under which the GPU comparison
(tests/test_gpu_dqn_direct.py) means something; (2) on every Double-DQN case the float32 and the float64 oracle pick the same arg-max
action of the online q(x2) on every row of every batch, and the float64 row's top two values are at least GAP apart: 1e-4 of the row's
largest |q|, a hundred times what a float32 forward of these depths loses — so a row whose arg-max flips on the GPU is a defect, not
a tie.  (A case that failed would be given another data seed in the case list.)"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _state_parity as sp  # noqa: E402
from _dqn_direct_cases import CASES  # noqa: E402

from oracle import dqn_oracle as do  # noqa: E402

GAP = 1e-4


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_direct_bars_are_a_tenth_of_the_movement_or_less(case):
    o64, _, o32, _ = sp.oracles(case)
    ratio = sp.bar_over_movement(o64, o32, sp.start_of(case), case.k)
    whole = {k: v for k, v in ratio.items() if k[1] == "*"}
    assert whole and all(v <= sp.MOVEMENT_SHARE for v in whole.values()), whole


class _Rec(do.DqnOracle):
    def forward_loss(self, batch, main=None, frozen=None):
        if frozen is None:      # (the evaluation whose backup is formed, not a re-evaluation against a frozen one)
            p = self.main if main is None else main
            self.__dict__.setdefault("qx2", []).append(do.q_net(p, "main", self._t(batch["obs2"])).detach().double())
        return super().forward_loss(batch, main, frozen)


@pytest.mark.parametrize("case", [c for c in CASES if c.family == "ddqn"], ids=repr)
def test_ddqn_argmax_is_no_tie(case):
    o64, _ = sp.run_oracle(case, torch.float64, cls=_Rec)
    o32, _ = sp.run_oracle(case, torch.float32, cls=_Rec)
    assert len(o64.qx2) >= case.updates and len(o64.qx2) == len(o32.qx2)
    for a, b in zip(o64.qx2, o32.qx2):
        assert torch.equal(a.argmax(1), b.argmax(1))
        top = a.topk(2, dim=1).values
        assert ((top[:, 0] - top[:, 1]) >= GAP * a.abs().max(1).values).all(), (top[:, 0] - top[:, 1]).min()
