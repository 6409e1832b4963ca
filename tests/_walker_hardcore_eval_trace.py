"""The env half of an evaluation trace on the HARDCORE WALKER (Actor.evaluate_env on an env.DeviceBipedalWalkerHardcore /
ddrl_env_eval_policy_walker_hardcore, csrc/walker_hardcore_eval.hip), shared by the CPU half (tests/test_walker_hardcore_eval_cpu.py)
and the GPU half (tests/test_gpu_walker_hardcore_eval.py): tests/_walker_eval_trace.py's functions with
tests/walker_hardcore_oracle.WalkerHardcoreOracle(1, seed, max_ep_len, vit, pit) positioned at `first_episode` in the oracle's place.

A trace row is the grass walker's: 32 floats — the observation acted on [0:24], the action [24:28], the reward [28], ended [29], then
two zeros [30:32]; rows past an episode's end are zero.  check_env_walker_hardcore feeds the recorded actions to the oracle episode
after episode; every recorded observation equals the oracle's observation before the step, the reward and ended equal the oracle's,
the lengths match, the return equals the float64 sum of the oracle's float32 rewards in step order, elements 30-31 are zero and so
are the rows past the end.  Everything is compared as bit patterns; there is no tolerance.

The policy half is _walker_eval_trace.check_policy as it is (model-independent: _acting_parity.actor_reference / compare on the played
rows, with the bars of _acting_parity).  No number is written here.

oracle_trace_walker_hardcore builds a trace from the oracles alone (_acting_parity.forward32 + WalkerHardcoreOracle) with one of
_eval_trace.DEFECTS planted; beside the trace it counts, per episode, the steps whose acted-on observation has a lidar ray that ends on
a box edge (the oracle's `last_ray_box` recording) — the steps on which the kernel's lidar reads the box rows of its LDS column."""
import numpy as np

import _acting_parity as ap
import _walker_eval_trace as wt
import walker_hardcore_oracle as who

F = np.float32
ROW, OBS, ACT, I_REW, I_END = wt.ROW, wt.OBS, wt.ACT, wt.I_REW, wt.I_END
WalkerEvalCase, params_of, played_rows, check_policy, _bits = wt.WalkerEvalCase, wt.params_of, wt.played_rows, wt.check_policy, wt._bits

# the GPU half's cases (seed 3, weight seeds 21 / 22: _walker_eval_trace's shapes replayed on the Hardcore oracle); the CPU half asserts
# on them what the GPU half relies on
TERMINAL_CASE = WalkerEvalCase("wh-64x48-n3-len120", (64, 48), 3, 120)                 # every episode ends on a terminal at step 54
WIDE_CASE = WalkerEvalCase("wh-400x300-n2-len120", (400, 300), 2, 120)                 # the full-width row; terminals at step 79
LIMIT_CASE = WalkerEvalCase("wh-ragged-70x44-n2-len120", (70, 44), 2, 120, wseed=22)   # h1 and h2 off 16; the time limit
ONE_STEP_CASE = WalkerEvalCase("wh-64x48-n1-len1", (64, 48), 1, 1)
GYM_CASE = WalkerEvalCase("wh-64x48-n1-len60-gym180x60", (64, 48), 1, 60, vit=180, pit=60)
FIRST_CASES = (WalkerEvalCase("wh-64x48-n8-len40", (64, 48), 8, 40), WalkerEvalCase("wh-64x48-n3-len40-first5", (64, 48), 3, 40, first=5))
TRACE_CASES = [TERMINAL_CASE, WIDE_CASE, LIMIT_CASE, ONE_STEP_CASE, GYM_CASE] + list(FIRST_CASES)
BOX_RAY_CASES = [TERMINAL_CASE, WIDE_CASE, LIMIT_CASE, GYM_CASE] + list(FIRST_CASES)   # a lidar ray ends on a box edge in each of these


def oracle_at(seed, first, max_ep_len, vit, pit):
    env = who.WalkerHardcoreOracle(1, seed, max_ep_len, vit, pit)
    env.S[who.EPI] = F(first)
    return env, env.reset()


def oracle_trace_walker_hardcore(case, params, defect=None, vit=None, pit=None):
    """The trace of `case` from _acting_parity.forward32 + WalkerHardcoreOracle alone, with ONE planted defect (_eval_trace.DEFECTS);
    vit / pit override the case's iteration counts (a trace played on another solver budget).  `box_steps` [n]: per episode, the steps
    acted on an observation with a lidar ray on a box edge."""
    cfg = ap.make_cfg(case.policy)
    vit, pit = (case.vit if vit is None else vit), (case.pit if pit is None else pit)
    n, L = case.n, case.max_ep_len
    limit = L + 1 if defect == "time_limit_one_step_late" else L
    ret, ln, trace, box = np.zeros(n), np.zeros(n, np.int32), np.zeros((n, L, ROW), F), np.zeros(n, np.int64)
    env, obs = oracle_at(case.seed, case.first, limit, vit, pit)
    for e in range(n):
        if defect == "episode_index_not_advanced":
            env, obs = oracle_at(case.seed, case.first, limit, vit, pit)
        total, total32, t, prev, ended = 0.0, F(0.0), 0, None, False
        while not ended:
            box[e] += int((env.last_ray_box != 0).any())      # of the lidar pass that made `obs`
            seen = prev if (defect == "action_from_previous_obs" and prev is not None) else obs
            act = ap.forward32(cfg, params, seen, np.zeros((1, ACT), F), defect if defect == "last_hidden2_dropped" else None)["mu"].astype(F)
            _, rew, _, nxt, end = env.step(act)
            ended = bool(end[0])
            if t < L:
                trace[e, t, :OBS], trace[e, t, OBS:OBS + ACT], trace[e, t, I_REW], trace[e, t, I_END] = obs[0], act[0], rew[0], F(ended)
            total, total32 = total + float(rew[0]), F(total32 + rew[0])
            prev, obs, t = obs, nxt, t + 1
        ret[e], ln[e] = (float(total32) if defect == "return_summed_in_float32" else total), t
    return dict(ret=ret, len=ln, trace=trace, box_steps=box)


def check_env_walker_hardcore(out, seed, first, max_ep_len, vit, pit, label=""):
    """_walker_eval_trace.check_env_walker on the Hardcore oracle; raises AssertionError with the first difference."""
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
