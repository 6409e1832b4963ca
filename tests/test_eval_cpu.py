"""CPU half of the evaluation-trace checks (tests/_eval_trace.py): on traces built from the oracles alone — _acting_parity.forward32
and LanderOracle — both checks pass, each of five planted defects fails at least one of them, and the fixed inputs of every case
meet the conditions the GPU half (tests/test_gpu_eval.py) relies on: an unsaturated policy and both kinds of episode end."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _acting_parity as ap  # noqa: E402
import _eval_trace as et  # noqa: E402

DEFECT_CASES = [c for c in et.TRACE_CASES if c.id in ("400x300-n4-len40", "400x300-n3-len400")]
_TRACES = {}


def _trace(case, defect=None):
    key = (case.id, defect)
    if key not in _TRACES:
        _TRACES[key] = et.oracle_trace(case, et.params_of(case), defect)
    return _TRACES[key]


def _fails(check, *a, **kw):
    try:
        check(*a, **kw)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("case", et.CASES, ids=repr)
def test_checks_pass_on_the_oracles_trace(case):
    out = _trace(case)
    et.check_env(out, case.seed, case.first, case.max_ep_len, case.id)
    et.check_policy(out, case, et.params_of(case))


@pytest.mark.parametrize("case", et.CASES, ids=repr)
def test_inputs_are_sensitive_and_end_both_ways(case):
    out = _trace(case)
    share = ap.sensitive_share(et.policy_reference(case, et.params_of(case), out))
    assert share >= ap.SENSITIVE_SHARE, "%s: %.3f of the action elements are unsaturated" % (case.id, share)
    last = np.array([out["trace"][e, l - 1] for e, l in enumerate(out["len"])])
    assert (last[:, 11] == 1).all()
    if case.max_ep_len == 40:     # every episode ends on the time limit
        assert (out["len"] == 40).all() and (last[:, 10] != -100).all()
    if case.max_ep_len == 400:    # at least one ends on a terminal before it
        assert ((out["len"] < 400) & (last[:, 10] == -100)).any()


@pytest.mark.parametrize("defect", et.DEFECTS)
@pytest.mark.parametrize("case", DEFECT_CASES, ids=repr)
def test_planted_defect_fails_a_check(case, defect):
    if defect == "episode_index_not_advanced":
        assert case.n > 1
    out, params = _trace(case, defect), et.params_of(case)
    if defect == "time_limit_one_step_late" and (_trace(case)["len"] < case.max_ep_len).all():
        # no episode of this case reaches the limit: by its definition the defect changes nothing here, and the trace says so
        assert all((np.asarray(out[k]) == np.asarray(_trace(case)[k])).all() for k in ("ret", "len", "trace"))
        return
    env_fails = _fails(et.check_env, out, case.seed, case.first, case.max_ep_len)
    pol_fails = _fails(et.check_policy, out, case, params)
    assert env_fails or pol_fails, "%s passes both checks on %s" % (defect, case.id)
    # each defect is seen by the half it belongs to
    if defect in ("action_from_previous_obs", "last_hidden2_dropped"):
        assert pol_fails
    else:
        assert env_fails


def test_first_episode_positions_the_stream():
    """Episodes 5.. of the n = 8 trace are the episodes 0.. of the first_episode = 5 trace."""
    long, short = _trace(et.FIRST_CASES[0]), _trace(et.FIRST_CASES[1])
    assert (long["trace"][5:8].view(np.uint32) == short["trace"].view(np.uint32)).all()
    assert (long["ret"][5:8] == short["ret"]).all() and (long["len"][5:8] == short["len"]).all()
