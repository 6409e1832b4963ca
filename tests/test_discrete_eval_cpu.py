"""CPU half of the discrete evaluation-trace checks (tests/_discrete_eval_trace.py): on traces built from the oracles alone — q_row32,
_discrete_acting.select and LanderOracle — the three checks pass, each of eight planted defects fails the check it belongs to, the
fixed inputs of every case meet the conditions the GPU half (tests/test_gpu_discrete_eval.py) relies on, and the float32 restatement
of the kernel's summation order is held to the float64 oracle (and to the same order written out as scalar loops)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _acting_parity as ap  # noqa: E402
import _discrete_eval_trace as dt  # noqa: E402

F = np.float32
BY_ID = {c.id: c for c in dt.CASES}
LEN40, LEN400, RAGGED = BY_ID["ddqn-400x300-g097-n4-len40"], BY_ID["ddqn-400x300-g05-n3-len400"], BY_ID["ddqn-ragged-70x44-g05-n3-len40"]
# defect -> (the cases it is planted in, the check that must see it)
PLANTED = {
    "action_from_previous_obs": ((LEN40, LEN400), "q"),
    "time_limit_one_step_late": ((LEN40, RAGGED), "env"),
    "return_summed_in_float32": ((LEN40, LEN400), "env"),
    "episode_index_not_advanced": ((LEN40, LEN400), "env"),
    "last_hidden2_dropped": ((LEN40, LEN400, RAGGED), "q"),
    "u1_from_next_step": ((LEN400, RAGGED), "actions"),          # greedy_prob 0.5: half of the rows take the random branch
    "argmax_takes_last_of_tie": ((dt.TIE_CASE,), "actions"),
    "head_bias_of_action_3_dropped": ((LEN40, LEN400, RAGGED), "q"),
}
_TRACES = {}


def _trace(case, defect=None):
    key = (case.id, defect)
    if key not in _TRACES:
        _TRACES[key] = dt.oracle_trace(case, dt.params_of(case), defect)
    return _TRACES[key]


def _fails(check, *a, **kw):
    try:
        check(*a, **kw)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("case", dt.CASES, ids=repr)
def test_checks_pass_on_the_oracles_trace(case):
    out = _trace(case)
    assert out["trace"].shape == (case.n, case.max_ep_len, dt.ROW)
    dt.check_all(out, case, dt.params_of(case))


def test_every_defect_is_planted():
    assert set(PLANTED) == set(dt.DEFECTS)


@pytest.mark.parametrize("defect,case", [(d, c) for d in dt.DEFECTS for c in PLANTED[d][0]], ids=lambda x: x if isinstance(x, str) else repr(x))
def test_planted_defect_fails_a_check(defect, case):
    out, params = _trace(case, defect), dt.params_of(case)
    fails = {"env": _fails(dt.check_env, out, case.seed, case.first, case.max_ep_len),
             "q": _fails(dt.check_q, out, case, params),
             "actions": _fails(dt.check_actions, out, case)}
    assert any(fails.values()), "%s passes all three checks on %s" % (defect, case.id)
    assert fails[PLANTED[defect][1]], "%s on %s: seen by %s, not by the check it belongs to" % (defect, case.id, [k for k, v in fails.items() if v])


@pytest.mark.parametrize("case", dt.CASES, ids=repr)
def test_inputs_end_both_ways_and_take_both_branches(case):
    out = _trace(case)
    rows = dt.played_rows(out)
    last = np.array([out["trace"][e, l - 1] for e, l in enumerate(out["len"])])
    assert (last[:, 18] == 1).all()
    if case.max_ep_len == 40:      # every episode ends on the time limit
        assert (out["len"] == 40).all() and (last[:, 17] != -100).all()
    if case.max_ep_len == 400:     # at least one ends on a terminal before it
        assert ((out["len"] < 400) & (last[:, 17] == -100)).any()
    if case.family == "ddqn" and not case.deterministic and case.greedy == 0.5:
        u0, _ = dt.call_uniforms(out, case.nseed, case.ctr, case.max_ep_len)
        assert (u0 < F(0.5)).any() and (u0 >= F(0.5)).any()
        assert len(set(rows[:, 16].tolist())) >= 3
    if case.family == "sqn" and not case.deterministic:
        # no row of the float32 restatement sits on a cumulative boundary: the exclusion rule of check_actions excludes nothing here
        assert int(dt.boundary_rows(out, case)[1].sum()) == 0
        assert len(set(rows[:, 16].tolist())) >= 2
    if case is dt.TIE_CASE:        # the copied columns hold the row maximum: a tie the selection has to break
        q = rows[:, 8:12]
        assert ((q[:, 1] == q[:, 2]) & (q[:, 1] >= q.max(axis=1))).sum() >= 8


def test_the_counter_crosses_2_to_the_32():
    c = LEN400     # inside a played episode: one of its steps draws below 2^32, a later one above
    starts = [c.ctr + 2 * e * c.max_ep_len for e in range(c.n)]
    assert any(s < (1 << 32) < s + 2 * int(l) - 2 for s, l in zip(starts, _trace(c)["len"]))


def _q_row_scalar(params, x):
    """The summation order of csrc/eval_q.hip's header as scalar float32 loops, one row."""
    W1, b1, W2, b2, W3, b3 = (np.asarray(params["main/q1/" + k], F) for k in
                              ("dense/kernel", "dense/bias", "dense_1/kernel", "dense_1/bias", "dense_2/kernel", "dense_2/bias"))
    h1, h2, A = b1.size, b2.size, b3.size
    h = np.zeros(h1, F)
    for j in range(h1):
        acc = b1[j]
        for q in range(8):
            acc = F(acc + F(x[q] * W1[q, j]))
        h[j] = max(acc, F(0))
    per, v = (h1 + 15) // 16, np.zeros(h2, F)
    for c in range(h2):
        total = b2[c]
        for s in range(16):
            acc = F(0)
            for k in range(s * per, min(s * per + per, h1)):
                acc = F(acc + F(h[k] * W2[k, c]))
            total = F(total + acc)
        v[c] = max(total, F(0))
    out = np.zeros(A, F)
    for a in range(A):
        total = F(0)
        for g in range((h2 + 15) // 16):
            acc = F(0)
            for c in range(16 * g, min(16 * g + 16, h2)):
                acc = F(acc + F(v[c] * W3[c, a]))
            total = F(total + acc)
        out[a] = F(total + b3[a])
    return out


@pytest.mark.parametrize("case", [RAGGED, BY_ID["sqn-64x32-det-n3-len40"]], ids=repr)
def test_restatement_equals_the_scalar_loops(case):
    params, obs = dt.params_of(case), dt.played_rows(_trace(case))[:3, :8]
    got = dt.q_row32(params, obs)
    for i in range(3):
        assert (got[i].view(np.uint32) == _q_row_scalar(params, obs[i]).view(np.uint32)).all(), (case.id, i)


@pytest.mark.parametrize("case", [LEN40, RAGGED, BY_ID["sqn-64x32-sample-n3-len40"]], ids=repr)
def test_restatement_against_the_float64_oracle(case):
    """q_row32 on fresh observations (not the trace's) within _acting_parity's bars of the float64 forward."""
    params = dt.params_of(case)
    obs = np.random.RandomState(case.wseed + 300).randn(64, 8).astype(F)
    ap.compare(dt.q_row32(params, obs), ap.q_reference(case.q, params, obs), "q1", case.id)
    with pytest.raises(AssertionError):
        ap.compare(dt.q_row32(params, obs, "head_bias_of_action_3_dropped"), ap.q_reference(case.q, params, obs), "q1", case.id)


def test_first_episode_positions_the_stream():
    """Episodes 5.. of the n = 8 trace are the episodes 0.. of the first_episode = 5 trace."""
    long, short = _trace(dt.FIRST_CASES[0]), _trace(dt.FIRST_CASES[1])
    assert (long["trace"][5:8].view(np.uint32) == short["trace"].view(np.uint32)).all()
    assert (long["ret"][5:8] == short["ret"]).all() and (long["len"][5:8] == short["len"]).all()


def test_two_calls_equal_one_split_at_the_counter():
    """Episodes 2, 3 of an n = 4 call are a call of n = 2 with first_episode = 2 at the counter 2 * 2 * max_ep_len further on."""
    c = dt.COUNTER_CASE
    whole = _trace(c)
    second = dt.DCase("second", c.family, c.hid, 2, c.max_ep_len, greedy=c.greedy, first=2, ctr=c.ctr + 2 * 2 * c.max_ep_len, wseed=c.wseed)
    out = dt.oracle_trace(second, dt.params_of(c))
    assert (whole["trace"][2:].view(np.uint32) == out["trace"].view(np.uint32)).all() and (whole["ret"][2:] == out["ret"]).all()
    dt.check_actions(out, second)
    assert _fails(dt.check_actions, out, second, ctr=c.ctr)      # ... and not at the first call's counter
