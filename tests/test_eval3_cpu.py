"""CPU half of the articulated lander's evaluation-trace checks (tests/_eval3_trace.py): on traces built from the oracles alone —
_acting_parity.forward32 and Lander3Oracle — check_env3 and _eval_trace.check_policy pass; each of the five planted defects of
_eval_trace.DEFECTS, a trace played on the one-body LanderOracle and a trace played with the velocity and position iteration counts
swapped are seen; and the fixed inputs meet the conditions the GPU half (tests/test_gpu_eval3.py) relies on: every episode of the
time-limit case ends on the limit, at least one episode of the long case ends on a terminal before it, and a leg touches ground.
Also: the header declares the three handle-fed entry points, the ctypes table lists them, the library exports them, and none of them
takes caller device memory."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _eval_trace as et  # noqa: E402
import _eval3_trace as e3  # noqa: E402

_TRACES = {}


def _trace(case, defect=None, swapped=False):
    key = (case.id, defect, swapped)
    if key not in _TRACES:
        kw = dict(vit=case.pit, pit=case.vit) if swapped else {}
        _TRACES[key] = e3.oracle_trace3(case, et.params_of(case), defect, **kw)
    return _TRACES[key]


def _fails(check, *a, **kw):
    try:
        check(*a, **kw)
    except AssertionError:
        return True
    return False


def _env_check(out, case):
    e3.check_env3(out, case.seed, case.first, case.max_ep_len, case.vit, case.pit, case.id)


@pytest.mark.parametrize("case", [e3.LIMIT_CASE, e3.LONG_CASE], ids=repr)
def test_checks_pass_on_the_oracles_trace(case):
    out = _trace(case)
    _env_check(out, case)
    et.check_policy(out, case, et.params_of(case))


def test_inputs_end_both_ways_and_touch_ground():
    short, long = _trace(e3.LIMIT_CASE), _trace(e3.LONG_CASE)
    last = lambda out: np.array([out["trace"][e, l - 1] for e, l in enumerate(out["len"])])
    assert (last(short)[:, 11] == 1).all() and (last(long)[:, 11] == 1).all()
    # every episode of the time-limit case ends on the limit
    assert (short["len"] == e3.LIMIT_CASE.max_ep_len).all() and (last(short)[:, 10] != -100).all()
    # at least one episode of the long case ends on a terminal before it
    assert ((long["len"] < e3.LONG_CASE.max_ep_len) & (last(long)[:, 10] == -100)).any(), long["len"]
    # at least one played step has a leg contact
    rows = et.played_rows(long)[0]
    assert ((rows[:, 6] == 1) | (rows[:, 7] == 1)).any()


@pytest.mark.parametrize("defect", et.DEFECTS)
def test_planted_defect_fails_a_check(defect):
    case = e3.LIMIT_CASE
    assert case.n > 1      # episode_index_not_advanced needs a second episode
    out, params = _trace(case, defect), et.params_of(case)
    env_fails = _fails(_env_check, out, case)
    pol_fails = _fails(et.check_policy, out, case, params)
    # each defect is seen by the half it belongs to
    if defect in ("action_from_previous_obs", "last_hidden2_dropped"):
        assert pol_fails, defect
    else:
        assert env_fails, defect


def test_a_trace_played_on_the_one_body_lander_is_seen():
    case = e3.LIMIT_CASE
    out = et.oracle_trace(case, et.params_of(case))      # LanderOracle, the same policy and streams
    et.check_env(out, case.seed, case.first, case.max_ep_len)      # ... a sound trace of that model
    assert _fails(_env_check, out, case)


def test_a_trace_played_with_the_iteration_counts_swapped_is_seen():
    case = e3.LONG_CASE
    assert case.vit != case.pit
    out = _trace(case, swapped=True)
    e3.check_env3(out, case.seed, case.first, case.max_ep_len, case.pit, case.vit, case.id)      # sound for the budget it was played on
    assert _fails(_env_check, out, case)


def test_header_signatures_and_exports_of_the_handle_fed_entry_points():
    from distributed_drl_amd import _lib
    import test_abi_table_cpu as tab
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "ddrl.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    names = ("ddrl_env_eval_policy", "ddrl_env_eval_q", "ddrl_env_eval_results")
    takes = tab.takes_device_memory(header)
    lib = _lib.load()      # loads on the CPU; no compute call
    for name in names:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
        assert name not in takes, (name, takes.get(name))
    assert len(_lib.SIGNATURES["ddrl_env_eval_policy"][1]) == 6 and len(_lib.SIGNATURES["ddrl_env_eval_q"][1]) == 10
    assert len(_lib.SIGNATURES["ddrl_env_eval_results"][1]) == 7
    # the two "no evaluation kernel yet" sentences are gone from the header
    assert "no evaluation kernel yet" not in header
