"""The two checks of an evaluation trace (Actor.evaluate(trace=True), csrc/eval.hip), shared by the CPU half
(tests/test_eval_cpu.py: both checks pass on a trace built from the oracles alone and see five planted defects) and the GPU half
(tests/test_gpu_eval.py: the device's traces are held to them).

A trace is what n deterministic evaluation episodes leave behind: ret [n] float64, len [n] int, trace [n, max_ep_len, 12] float32 with
per step the observation acted on [0:8], the action [8:10], the reward [10] and ended [11]; rows past an episode's end are zero.

(a) ENV HALF, bit for bit.  The recorded actions are fed, episode after episode, to oracle.env_oracle.LanderOracle(1, seed,
    max_ep_len) positioned at `first_episode` (S[EPI] set, then reset()).  Every recorded observation equals the oracle's
    observation before the step, the reward and ended equal the oracle's, the lengths match, the return equals the float64 sum of
    the oracle's float32 rewards in step order, rows past the end are zero.  Floats are compared as bit patterns.
(b) POLICY HALF.  The recorded actions are held to tests/_acting_parity.actor_reference(...) kind "mu" evaluated on the recorded
    observations, through _acting_parity.compare with the bars that file computes (K = 2 over the float32 ensemble, resolution term
    2^-22).  No tolerance is written here.

INPUTS  glorot kernels with the non-zero biases of _acting_parity.make_params; the weight seed of every case is fixed below and the
        CPU half checks the sensitivity rule of _acting_parity on it (>= 90 % of the trace's action elements have 1 - a64^2 >= 0.1)
        and that both endings occur: every episode of a max_ep_len = 40 case ends on the time limit, at least one episode of the
        max_ep_len = 400 case ends on a terminal (rew == -100) before it."""
import numpy as np

import _acting_parity as ap
from oracle import env_oracle as eo

ROW = 12
F = np.float32


class EvalCase:
    """n episodes from `first` on of the env stream `seed`, policy of hidden sizes `hid` with weight seed `wseed`."""

    def __init__(self, id, hid, n, max_ep_len, first=0, seed=3, wseed=21):
        self.id, self.hid, self.n, self.max_ep_len, self.first, self.seed, self.wseed = id, tuple(hid), n, max_ep_len, first, seed, wseed
        self.policy = ap.Case(id, 8, 2, hid, rows=1, direct=False, seed=wseed)

    def __repr__(self):
        return self.id


TRACE_CASES = [
    EvalCase("400x300-n4-len40", (400, 300), 4, 40),
    EvalCase("400x300-n3-len400", (400, 300), 3, 400),
    EvalCase("400x300-n1-len1", (400, 300), 1, 1),
    EvalCase("ragged-70x44-n3-len40", (70, 44), 3, 40, wseed=22),   # h1 and h2 off 16: the slice and column-group tails
]
FIRST_CASES = (EvalCase("400x300-n8-len40", (400, 300), 8, 40), EvalCase("400x300-n3-len40-first5", (400, 300), 3, 40, first=5))
CASES = TRACE_CASES + list(FIRST_CASES)
DEFECTS = ("action_from_previous_obs", "time_limit_one_step_late", "return_summed_in_float32", "episode_index_not_advanced",
           "last_hidden2_dropped")


def params_of(case):
    return ap.make_params(case.policy)


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, F)).view(np.uint32)


def _oracle_at(seed, first, max_ep_len):
    env = eo.LanderOracle(1, seed, max_ep_len)
    env.S[eo.EPI] = F(first)
    return env, env.reset()


def oracle_trace(case, params, defect=None):
    """The trace of `case` from the oracles alone: _acting_parity.forward32 (float32 policy) + LanderOracle, with ONE planted defect."""
    cfg = ap.make_cfg(case.policy)
    n, L = case.n, case.max_ep_len
    limit = L + 1 if defect == "time_limit_one_step_late" else L
    ret, ln, trace = np.zeros(n), np.zeros(n, np.int32), np.zeros((n, L, ROW), F)
    env, obs = _oracle_at(case.seed, case.first, limit)
    for e in range(n):
        if defect == "episode_index_not_advanced":
            env, obs = _oracle_at(case.seed, case.first, limit)
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


def check_env(out, seed, first, max_ep_len, label=""):
    """(a) of the module docstring; raises AssertionError with the first difference."""
    ret, ln, trace = np.asarray(out["ret"], np.float64), np.asarray(out["len"]), np.asarray(out["trace"], F)
    n = trace.shape[0]
    assert trace.shape == (n, max_ep_len, ROW) and ret.shape == (n,) and ln.shape == (n,), "%s: shapes %s %s %s" % (label, trace.shape, ret.shape, ln.shape)
    env, obs = _oracle_at(seed, first, max_ep_len)
    for e in range(n):
        total, t, ended = 0.0, 0, False
        while not ended:
            where = "%s episode %d step %d" % (label, e, t)
            assert t < max_ep_len and t < ln[e], "%s: the oracle's episode goes on past the recorded length %d" % (where, ln[e])
            row = trace[e, t]
            assert (_bits(row[:8]) == _bits(obs[0])).all(), "%s: observation %r, oracle %r" % (where, row[:8], obs[0])
            _, rew, _, obs, end = env.step(row[8:10].reshape(1, 2))
            ended = bool(end[0])
            assert _bits(row[10]) == _bits(rew[0]), "%s: reward %r, oracle %r" % (where, row[10], rew[0])
            assert _bits(row[11]) == _bits(F(ended)), "%s: ended %r, oracle %r" % (where, row[11], ended)
            total, t = total + float(rew[0]), t + 1
        assert ln[e] == t, "%s episode %d: length %d, oracle %d" % (label, e, ln[e], t)
        assert ret[e] == total, "%s episode %d: return %r, float64 sum of the oracle's float32 rewards %r" % (label, e, ret[e], total)
        assert not _bits(trace[e, t:]).any(), "%s episode %d: rows past the end are not zero" % (label, e)


def played_rows(out):
    """(observations [steps, 8], actions [steps, 2]) of every step played, episode after episode."""
    trace = np.asarray(out["trace"], F)
    rows = np.concatenate([trace[e, :int(l)] for e, l in enumerate(out["len"])])
    return rows[:, :8], rows[:, 8:10]


def policy_reference(case, params, out):
    return ap.actor_reference(case.policy, [params], None, played_rows(out)[0], None)


def check_policy(out, case, params, label="", table=None, ref=None):
    """(b) of the module docstring."""
    ref = policy_reference(case, params, out) if ref is None else ref
    ap.compare(played_rows(out)[1], ref, "mu", label or case.id, table=table)
