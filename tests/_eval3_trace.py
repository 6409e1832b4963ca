"""The env half of an evaluation trace on the ARTICULATED lander (Actor.evaluate_env / ddrl_env_eval_policy and dqn.Actor.evaluate_env /
ddrl_env_eval_q, csrc/eval3.hip), shared by the CPU half (tests/test_eval3_cpu.py) and the GPU half (tests/test_gpu_eval3.py).

check_env3 is tests/_eval_trace.check_env with tests/lander3_oracle.Lander3Oracle(1, seed, max_ep_len, vit, pit) positioned at
`first_episode` in the place of LanderOracle: the recorded actions are fed to the oracle episode after episode; every recorded
observation equals the oracle's observation before the step, the reward and ended equal the oracle's, the lengths match, the return
equals the float64 sum of the oracle's float32 rewards in step order, rows past the end are zero.  Everything is compared as bit
patterns; there is no tolerance.  check_env3_discrete is the same on the 20-float rows of the discrete trace, the recorded action
indices going through the oracle's discrete action table (_discrete_acting.table_actions: gym's, the one ddrl_env_step_discrete uses).

The policy and Q-row halves are model-independent: _eval_trace.check_policy and _discrete_eval_trace.check_q / check_actions are
reused as they are, with the bars of _acting_parity.  No number is written here.

oracle_trace3 builds a continuous trace from the oracles alone (_acting_parity.forward32 + Lander3Oracle) with one of
_eval_trace.DEFECTS planted, as _eval_trace.oracle_trace does on the one-body oracle."""
import numpy as np

import _acting_parity as ap
import _discrete_acting as da
import _eval_trace as et
import lander3_oracle as l3

F = np.float32
ROW, ROW_Q = 12, 20


class Eval3Case(et.EvalCase):
    """An _eval_trace.EvalCase plus the solver's iteration counts."""

    def __init__(self, id, hid, n, max_ep_len, vit=8, pit=3, **kw):
        super().__init__(id, hid, n, max_ep_len, **kw)
        self.vit, self.pit = vit, pit


# the GPU half's continuous cases (tests/test_gpu_eval3.py); the CPU half asserts on the first two what the GPU half relies on
TRACE_CASES = [
    Eval3Case("a-64x48-n3-len120", (64, 48), 3, 120),                      # terminals and leg contacts
    Eval3Case("a-400x300-n2-len40", (400, 300), 2, 40),                    # the full-width row; every episode ends on the time limit
    Eval3Case("a-ragged-70x44-n2-len30", (70, 44), 2, 30, wseed=22),       # h1 and h2 off 16: the slice and column-group tails
    Eval3Case("a-64x48-n1-len1", (64, 48), 1, 1),
    Eval3Case("a-64x48-n2-len12-gym180x60", (64, 48), 2, 12, vit=180, pit=60),
]
FIRST_CASES = (Eval3Case("a-64x48-n8-len40", (64, 48), 8, 40), Eval3Case("a-64x48-n3-len40-first5", (64, 48), 3, 40, first=5))
# the CPU half: both endings at the GPU half's iteration counts (8 / 3)
LIMIT_CASE = Eval3Case("a-64x48-n2-len40", (64, 48), 2, 40)
LONG_CASE = TRACE_CASES[0]


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, F)).view(np.uint32)


def oracle_at(seed, first, max_ep_len, vit, pit):
    env = l3.Lander3Oracle(1, seed, max_ep_len, vit, pit)
    env.S[l3.EPI] = F(first)
    return env, env.reset()


def oracle_trace3(case, params, defect=None, vit=None, pit=None):
    """The trace of `case` from _acting_parity.forward32 + Lander3Oracle alone, with ONE planted defect (_eval_trace.DEFECTS);
    vit / pit override the case's iteration counts (a trace played on another solver budget)."""
    cfg = ap.make_cfg(case.policy)
    vit, pit = (case.vit if vit is None else vit), (case.pit if pit is None else pit)
    n, L = case.n, case.max_ep_len
    limit = L + 1 if defect == "time_limit_one_step_late" else L
    ret, ln, trace = np.zeros(n), np.zeros(n, np.int32), np.zeros((n, L, ROW), F)
    env, obs = oracle_at(case.seed, case.first, limit, vit, pit)
    for e in range(n):
        if defect == "episode_index_not_advanced":
            env, obs = oracle_at(case.seed, case.first, limit, vit, pit)
        total, total32, t, prev, ended = 0.0, F(0.0), 0, None, False
        while not ended:
            seen = prev if (defect == "action_from_previous_obs" and prev is not None) else obs
            act = ap.forward32(cfg, params, seen, np.zeros((1, 2), F), defect if defect == "last_hidden2_dropped" else None)["mu"].astype(F)
            _, rew, _, nxt, end = env.step(act)
            ended = bool(end[0])
            if t < L:
                trace[e, t, :8], trace[e, t, 8:10], trace[e, t, 10], trace[e, t, 11] = obs[0], act[0], rew[0], F(ended)
            total, total32 = total + float(rew[0]), F(total32 + rew[0])
            prev, obs, t = obs, nxt, t + 1
        ret[e], ln[e] = (float(total32) if defect == "return_summed_in_float32" else total), t
    return dict(ret=ret, len=ln, trace=trace)


def _check(out, seed, first, max_ep_len, vit, pit, label, row_len, action_of, i_rew, i_end, extra=None):
    ret, ln, trace = np.asarray(out["ret"], np.float64), np.asarray(out["len"]), np.asarray(out["trace"], F)
    n = trace.shape[0]
    assert trace.shape == (n, max_ep_len, row_len) and ret.shape == (n,) and ln.shape == (n,), "%s: shapes %s %s %s" % (label, trace.shape, ret.shape, ln.shape)
    env, obs = oracle_at(seed, first, max_ep_len, vit, pit)
    for e in range(n):
        total, t, ended = 0.0, 0, False
        while not ended:
            where = "%s episode %d step %d" % (label, e, t)
            assert t < max_ep_len and t < ln[e], "%s: the oracle's episode goes on past the recorded length %d" % (where, ln[e])
            row = trace[e, t]
            assert (_bits(row[:8]) == _bits(obs[0])).all(), "%s: observation %r, oracle %r" % (where, row[:8], obs[0])
            if extra is not None:
                extra(row, where)
            _, rew, _, obs, end = env.step(action_of(row))
            ended = bool(end[0])
            assert _bits(row[i_rew]) == _bits(rew[0]), "%s: reward %r, oracle %r" % (where, row[i_rew], rew[0])
            assert _bits(row[i_end]) == _bits(F(ended)), "%s: ended %r, oracle %r" % (where, row[i_end], ended)
            total, t = total + float(rew[0]), t + 1
        assert ln[e] == t, "%s episode %d: length %d, oracle %d" % (label, e, ln[e], t)
        assert ret[e] == total, "%s episode %d: return %r, float64 sum of the oracle's float32 rewards %r" % (label, e, ret[e], total)
        assert not _bits(trace[e, t:]).any(), "%s episode %d: rows past the end are not zero" % (label, e)


def check_env3(out, seed, first, max_ep_len, vit, pit, label=""):
    """_eval_trace.check_env on the articulated oracle; raises AssertionError with the first difference."""
    _check(out, seed, first, max_ep_len, vit, pit, label, ROW, lambda row: row[8:10].reshape(1, 2), 10, 11)


def check_env3_discrete(out, seed, first, max_ep_len, vit, pit, label=""):
    """_discrete_eval_trace.check_env on the articulated oracle: the recorded indices go through the discrete action table."""
    def index_only(row, where):
        assert row[16] == np.trunc(row[16]) and row[16] >= 0, "%s: action %r is no index" % (where, row[16])
        assert _bits(row[19]) == 0, "%s: element 19 is %r" % (where, row[19])
    _check(out, seed, first, max_ep_len, vit, pit, label, ROW_Q, lambda row: da.table_actions(row[16:17]), 17, 18, index_only)
