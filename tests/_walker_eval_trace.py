"""The env half of an evaluation trace on the WALKER (Actor.evaluate_env on an env.DeviceBipedalWalker / ddrl_env_eval_policy_walker,
csrc/walker_eval.hip), shared by the CPU half (tests/test_walker_eval_cpu.py) and the GPU half (tests/test_gpu_walker_eval.py), in the
form of tests/_eval3_trace.py.

A trace row is 32 floats: the observation acted on [0:24], the action [24:28], the reward [28], ended [29], then two zeros [30:32];
rows past an episode's end are zero.

check_env_walker is tests/_eval_trace.check_env with tests/walker_oracle.WalkerOracle(1, seed, max_ep_len, vit, pit) positioned at
`first_episode` in the place of LanderOracle: the recorded actions are fed to the oracle episode after episode; every recorded
observation equals the oracle's observation before the step, the reward and ended equal the oracle's, the lengths match, the return
equals the float64 sum of the oracle's float32 rewards in step order, elements 30-31 are zero and so are the rows past the end.
Everything is compared as bit patterns; there is no tolerance.

The policy half is model-independent: _acting_parity.actor_reference / compare on the played rows, with the bars of _acting_parity.
No number is written here.

oracle_trace_walker builds a trace from the oracles alone (_acting_parity.forward32 + WalkerOracle) with one of _eval_trace.DEFECTS
planted, as _eval_trace.oracle_trace does on the one-body oracle."""
import numpy as np

import _acting_parity as ap
import _eval_trace as et
import walker_oracle as wo

F = np.float32
ROW, OBS, ACT = 32, wo.OBS, wo.ACT
I_REW, I_END = 28, 29


class WalkerEvalCase:
    """n episodes from `first` on of the env stream `seed` at `vit` / `pit` iterations, policy of hidden sizes `hid` with weight seed
    `wseed`."""

    def __init__(self, id, hid, n, max_ep_len, vit=8, pit=3, first=0, seed=3, wseed=21):
        self.id, self.hid, self.n, self.max_ep_len, self.first, self.seed, self.wseed = id, tuple(hid), n, max_ep_len, first, seed, wseed
        self.vit, self.pit = vit, pit
        self.policy = ap.Case(id, OBS, ACT, hid, rows=1, direct=False, seed=wseed)

    def __repr__(self):
        return self.id


# the GPU half's cases; the CPU half asserts on the first three what the GPU half relies on
TERMINAL_CASE = WalkerEvalCase("w-64x48-n3-len120", (64, 48), 3, 120)                 # every episode ends on a terminal, legs on the ground
WIDE_CASE = WalkerEvalCase("w-400x300-n2-len120", (400, 300), 2, 120)                 # the full-width row; terminals
LIMIT_CASE = WalkerEvalCase("w-ragged-70x44-n2-len120", (70, 44), 2, 120, wseed=22)   # h1 and h2 off 16; the time limit, long contact
TRACE_CASES = [
    TERMINAL_CASE, WIDE_CASE, LIMIT_CASE,
    WalkerEvalCase("w-64x48-n1-len1", (64, 48), 1, 1),
    WalkerEvalCase("w-64x48-n2-len12-gym180x60", (64, 48), 2, 12, vit=180, pit=60),
]
FIRST_CASES = (WalkerEvalCase("w-64x48-n8-len40", (64, 48), 8, 40), WalkerEvalCase("w-64x48-n3-len40-first5", (64, 48), 3, 40, first=5))


def params_of(case):
    return ap.make_params(case.policy)


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, F)).view(np.uint32)


def oracle_at(seed, first, max_ep_len, vit, pit):
    env = wo.WalkerOracle(1, seed, max_ep_len, vit, pit)
    env.S[wo.EPI] = F(first)
    return env, env.reset()


def oracle_trace_walker(case, params, defect=None, vit=None, pit=None):
    """The trace of `case` from _acting_parity.forward32 + WalkerOracle alone, with ONE planted defect (_eval_trace.DEFECTS);
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
            act = ap.forward32(cfg, params, seen, np.zeros((1, ACT), F), defect if defect == "last_hidden2_dropped" else None)["mu"].astype(F)
            _, rew, _, nxt, end = env.step(act)
            ended = bool(end[0])
            if t < L:
                trace[e, t, :OBS], trace[e, t, OBS:OBS + ACT], trace[e, t, I_REW], trace[e, t, I_END] = obs[0], act[0], rew[0], F(ended)
            total, total32 = total + float(rew[0]), F(total32 + rew[0])
            prev, obs, t = obs, nxt, t + 1
        ret[e], ln[e] = (float(total32) if defect == "return_summed_in_float32" else total), t
    return dict(ret=ret, len=ln, trace=trace)


def check_env_walker(out, seed, first, max_ep_len, vit, pit, label=""):
    """_eval_trace.check_env on the walker's oracle; raises AssertionError with the first difference."""
    ret, ln, trace = np.asarray(out["ret"], np.float64), np.asarray(out["len"]), np.asarray(out["trace"], F)
    n = trace.shape[0]
    assert trace.shape == (n, max_ep_len, ROW) and ret.shape == (n,) and ln.shape == (n,), "%s: shapes %s %s %s" % (label, trace.shape, ret.shape, ln.shape)
    env, obs = oracle_at(seed, first, max_ep_len, vit, pit)
    for e in range(n):
        total, t, ended = 0.0, 0, False
        while not ended:
            where = "%s episode %d step %d" % (label, e, t)
            assert t < max_ep_len and t < ln[e], "%s: the oracle's episode goes on past the recorded length %d" % (where, ln[e])
            row = trace[e, t]
            assert (_bits(row[:OBS]) == _bits(obs[0])).all(), "%s: observation %r, oracle %r" % (where, row[:OBS], obs[0])
            assert not _bits(row[30:32]).any(), "%s: elements 30-31 are %r" % (where, row[30:32])
            _, rew, _, obs, end = env.step(row[OBS:OBS + ACT].reshape(1, ACT))
            ended = bool(end[0])
            assert _bits(row[I_REW]) == _bits(rew[0]), "%s: reward %r, oracle %r" % (where, row[I_REW], rew[0])
            assert _bits(row[I_END]) == _bits(F(ended)), "%s: ended %r, oracle %r" % (where, row[I_END], ended)
            total, t = total + float(rew[0]), t + 1
        assert ln[e] == t, "%s episode %d: length %d, oracle %d" % (label, e, ln[e], t)
        assert ret[e] == total, "%s episode %d: return %r, float64 sum of the oracle's float32 rewards %r" % (label, e, ret[e], total)
        assert not _bits(trace[e, t:]).any(), "%s episode %d: rows past the end are not zero" % (label, e)


def played_rows(out):
    """(observations [steps, 24], actions [steps, 4]) of every step played, episode after episode."""
    trace = np.asarray(out["trace"], F)
    rows = np.concatenate([trace[e, :int(l)] for e, l in enumerate(out["len"])])
    return rows[:, :OBS], rows[:, OBS:OBS + ACT]


def check_policy(out, case, params, label="", table=None):
    """The recorded actions held to _acting_parity.actor_reference(...) kind "mu" evaluated on the recorded observations, through
    _acting_parity.compare with the bars that file computes."""
    obs, act = played_rows(out)
    ref = ap.actor_reference(case.policy, [params], None, obs, None)
    ap.compare(act, ref, "mu", label or case.id, table=table)
