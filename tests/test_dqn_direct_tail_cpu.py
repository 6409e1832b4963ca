"""CPU side of the direct-operand tail's tests (ddrl_dqn_create_direct_tail): the C ABI's door of its own — include/ddrl_dqn_direct_tail.h
against _lib.SIGNATURES_DQN_DIRECT_TAIL and the library's exports — and, on the two oracles alone as tests/test_dqn_direct_cpu.py does
for the narrow cases, (1) every case of tests/_dqn_direct_tail_cases.py keeps its whole-vector state bars at a tenth of the float64
oracle's movement or less, (2) no Double-DQN case sits on an arg-max tie (that file's recorder and GAP)."""
import ctypes
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _state_parity as sp  # noqa: E402
import test_dqn_direct_cpu as dc  # noqa: E402
from _dqn_direct_tail_cases import CASES  # noqa: E402

from distributed_drl_amd import _lib  # noqa: E402

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "ddrl_dqn_direct_tail.h")


def test_header_table_and_library_agree():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(ddrl_\w+)\s*\(", text))
    table = _lib.SIGNATURES_DQN_DIRECT_TAIL
    assert declared == set(table) == {"ddrl_dqn_create_direct_tail", "ddrl_dqn_is_direct_tail"}
    assert not set(table) & (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_DQN_DIRECT))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(lib, name) for name in table)
    assert table["ddrl_dqn_create_direct_tail"] == _lib.SIGNATURES["ddrl_dqn_create"]
    assert table["ddrl_dqn_is_direct_tail"] == _lib.SIGNATURES["ddrl_dqn_wide_sk"]


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_tail_bars_are_a_tenth_of_the_movement_or_less(case):
    o64, _, o32, _ = sp.oracles(case)
    ratio = sp.bar_over_movement(o64, o32, sp.start_of(case), case.k)
    whole = {k: v for k, v in ratio.items() if k[1] == "*"}
    assert whole and all(v <= sp.MOVEMENT_SHARE for v in whole.values()), whole


@pytest.mark.parametrize("case", [c for c in CASES if c.family == "ddqn"], ids=repr)
def test_ddqn_argmax_is_no_tie(case):
    o64, _ = sp.run_oracle(case, torch.float64, cls=dc._Rec)
    o32, _ = sp.run_oracle(case, torch.float32, cls=dc._Rec)
    assert len(o64.qx2) >= case.updates and len(o64.qx2) == len(o32.qx2)
    for a, b in zip(o64.qx2, o32.qx2):
        assert torch.equal(a.argmax(1), b.argmax(1))
        top = a.topk(2, dim=1).values
        assert ((top[:, 0] - top[:, 1]) >= dc.GAP * a.abs().max(1).values).all(), (top[:, 0] - top[:, 1]).min()
