"""The three checks of a discrete evaluation trace (dqn.Actor.evaluate(trace=True) / ddrl_dqn_eval, csrc/eval_q.hip), shared by the
CPU half (tests/test_discrete_eval_cpu.py: the checks pass on traces built from q_row32 + _discrete_acting.select + LanderOracle alone
and see eight planted defects) and the GPU half (tests/test_gpu_discrete_eval.py: the device's traces are held to them).

A trace is what n evaluation episodes leave behind: ret [n] float64, len [n] int, trace [n, max_ep_len, 20] float32 with per step the
observation acted on [0:8], the q row [8:16] (zeros beyond A), the action index [16], the reward [17], ended [18] and 0 [19]; rows past
an episode's end are zero.

(a) check_env, bit for bit.  The recorded action indices, mapped through _discrete_acting.table_actions, are fed episode after episode
    to oracle.env_oracle.LanderOracle(1, seed, max_ep_len) positioned at `first_episode`.  Observations, rewards, ended, lengths, the
    float64 returns (sum of the oracle's float32 rewards in step order) and the zero rows are compared as bit patterns.
(b) check_q.  The recorded q rows equal q_row32 — the kernel's summation order restated in NumPy float32, every product and every sum
    rounded separately — of the recorded observations bit for bit, and pass _acting_parity.compare(..., "q1", ...) against
    _acting_parity.q_reference on those observations (float64 oracle, the float32 ensemble as the yardstick).  No tolerance is written
    here.
(c) check_actions.  The recorded actions equal _discrete_acting.select on the trace's OWN recorded q rows with
    _discrete_acting.uniforms at the counters of the call: step t of episode e owns u0 = U(seed, ctr + 2 (e max_ep_len + t)) and
    u1 = U(seed, ctr + 2 (e max_ep_len + t) + 1).  Exact for Double-DQN and for SQN in deterministic mode; for SQN sampling the rule of
    tests/test_gpu_discrete_rollout.py: a row may be left out only if u0 * total lies within 1e-5 relative of a float64 cumulative
    boundary, and at most 1 % of the rows may (asserted).

SUMMATION ORDER of q_row32 (the header of csrc/eval_q.hip): layer-1 unit j = the bias, then + x[q] * W1[q][j] in input order; layer-2
column c = 16 slices of ceil(h1 / 16) contraction rows, each summed in row order from zero, added in slice order on the bias; head
partials per group of 16 columns in column order from zero, the groups added in group order from zero, then the head bias.

INPUTS  glorot kernels with the non-zero biases of _acting_parity.q_params; the weight seed of every case is fixed below, and the CPU
        half asserts on it what the GPU half relies on: both kinds of episode end, both branches of the coin flip, at least three of
        the four actions, no SQN row on a cumulative boundary."""
import numpy as np

import _acting_parity as ap
import _discrete_acting as da
from oracle import env_oracle as eo

ROW = 20
F = np.float32
MAX_EXCLUDED = 0.01      # tests/test_gpu_discrete_rollout.py's cap on boundary rows of SQN sampling


class DCase:
    """n episodes from `first` on of the env stream `seed`; a Q network of hidden sizes `hid` with weight seed `wseed`; the selection's
    mode and the (noise seed, counter) the call starts at."""

    def __init__(self, id, family, hid, n, max_ep_len, deterministic=False, greedy=0.97, alpha=0.1, first=0, seed=3, wseed=21,
                 nseed=0xC0FFEE, ctr=0, acts=4):
        self.id, self.family, self.hid, self.n, self.max_ep_len, self.deterministic = id, family, tuple(hid), n, max_ep_len, deterministic
        self.greedy, self.alpha, self.first, self.seed, self.wseed, self.nseed, self.ctr, self.acts = greedy, alpha, first, seed, wseed, nseed, ctr, acts
        self.q = ap.QCase(id, family, 8, acts, hid, 1, alpha=alpha, seed=wseed)

    def __repr__(self):
        return self.id


TRACE_CASES = [
    DCase("ddqn-400x300-g097-n4-len40", "ddqn", (400, 300), 4, 40, greedy=0.97, ctr=1000),
    DCase("ddqn-400x300-g05-n3-len400", "ddqn", (400, 300), 3, 400, greedy=0.5, ctr=(1 << 32) - 850),     # the counter crosses 2^32
    DCase("ddqn-400x300-det-n1-len1", "ddqn", (400, 300), 1, 1, deterministic=True),
    DCase("ddqn-ragged-70x44-g05-n3-len40", "ddqn", (70, 44), 3, 40, greedy=0.5, wseed=22, ctr=6),         # h1, h2 off 16: the tails
    DCase("sqn-64x32-det-n3-len40", "sqn", (64, 32), 3, 40, deterministic=True, wseed=23),
    DCase("sqn-64x32-sample-n3-len40", "sqn", (64, 32), 3, 40, alpha=0.1, wseed=23, ctr=250),
]
FIRST_CASES = (DCase("ddqn-400x300-det-n8-len40", "ddqn", (400, 300), 8, 40, deterministic=True),
               DCase("ddqn-400x300-det-n3-len40-first5", "ddqn", (400, 300), 3, 40, deterministic=True, first=5))
COUNTER_CASE = DCase("ddqn-400x300-g05-n4-len40", "ddqn", (400, 300), 4, 40, greedy=0.5, ctr=77)
# last-layer columns 1 and 2 are copies (bias included, lifted above the others): the row maximum is a tie wherever they hold it
TIE_CASE = DCase("ddqn-400x300-det-n1-len40-tied", "ddqn", (400, 300), 1, 40, deterministic=True)
# beyond the lander's four actions (indices above 3 clamp to the table's last entry): the head's A = 8 limit and an odd A
WIDE_CASES = [DCase("ddqn-ragged-70x44-a8-g05-n2-len40", "ddqn", (70, 44), 2, 40, greedy=0.5, wseed=24, ctr=12, acts=8),
              DCase("sqn-64x32-a3-sample-n2-len40", "sqn", (64, 32), 2, 40, alpha=0.1, wseed=25, ctr=90, acts=3)]
CASES = TRACE_CASES + list(FIRST_CASES) + [COUNTER_CASE, TIE_CASE] + WIDE_CASES
DEFECTS = ("action_from_previous_obs", "time_limit_one_step_late", "return_summed_in_float32", "episode_index_not_advanced",
           "last_hidden2_dropped", "u1_from_next_step", "argmax_takes_last_of_tie", "head_bias_of_action_3_dropped")


def params_of(case):
    params = ap.q_params(case.q)
    if case is TIE_CASE:
        for q in case.q.nets:
            k, b = params["main/%s/dense_2/kernel" % q].copy(), params["main/%s/dense_2/bias" % q].copy()
            k[:, 2], b[1] = k[:, 1], b[1] + 0.3
            b[2] = b[1]
            params["main/%s/dense_2/kernel" % q], params["main/%s/dense_2/bias" % q] = k, b
    return params


def q_row32(params, obs, defect=None):
    """q1 of obs [n, 8] in float32 in the kernel's summation order (module docstring): elementwise NumPy float32 operations only, so
    every product and every sum is rounded on its own.  `defect`: "last_hidden2_dropped" / "head_bias_of_action_3_dropped"."""
    W1, b1, W2, b2, W3, b3 = (np.asarray(params["main/q1/" + k], F) for k in
                              ("dense/kernel", "dense/bias", "dense_1/kernel", "dense_1/bias", "dense_2/kernel", "dense_2/bias"))
    x = np.asarray(obs, F).reshape(-1, 8)
    n, h1, h2, A = x.shape[0], b1.size, b2.size, b3.size
    acc = np.repeat(b1[None, :], n, axis=0)
    for q in range(8):                                   # input order, on the bias
        acc = acc + x[:, q:q + 1] * W1[q][None, :]
    h = np.maximum(acc, F(0.0))
    per = (h1 + 15) // 16
    sl = np.zeros((n, 16, h2), F)                        # the 16 slice sums of every column, each in row order from zero
    for i in range(per):
        rows = np.arange(16) * per + i
        s = np.nonzero(rows < h1)[0]                     # (a slice past h1 is empty)
        r = rows[s]
        sl[:, s, :] = sl[:, s, :] + h[:, r, None] * W2[r][None, :, :]
    acc = np.repeat(b2[None, :], n, axis=0)
    for s in range(16):                                  # slice order, on the bias
        acc = acc + sl[:, s, :]
    v = np.maximum(acc, F(0.0))
    if defect == "last_hidden2_dropped":                 # the last unit that is on for any row
        v = v.copy()
        v[:, int(np.nonzero(np.abs(v).sum(0) > 0)[0][-1])] = 0
    ng = (h2 + 15) // 16
    part = np.zeros((n, ng, A), F)                       # head partials per group of 16 columns, in column order from zero
    for i in range(16):
        cols = np.arange(ng) * 16 + i
        g = np.nonzero(cols < h2)[0]
        c = cols[g]
        part[:, g, :] = part[:, g, :] + v[:, c, None] * W3[c][None, :, :]
    q = np.zeros((n, A), F)
    for g in range(ng):                                  # group order, from zero
        q = q + part[:, g, :]
    bias = b3.copy()
    if defect == "head_bias_of_action_3_dropped":
        bias[3] = 0
    return (q + bias[None, :]).astype(F)


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, F)).view(np.uint32)


def _oracle_at(seed, first, max_ep_len):
    env = eo.LanderOracle(1, seed, max_ep_len)
    env.S[eo.EPI] = F(first)
    return env, env.reset()


def _last_max(q):
    q = np.asarray(q, F)
    return q.shape[1] - 1 - np.argmax(q[:, ::-1], axis=1)


def oracle_trace(case, params, defect=None):
    """The trace of `case` from q_row32 + _discrete_acting.select + LanderOracle alone, with ONE planted defect."""
    n, L, A = case.n, case.max_ep_len, case.acts
    limit = L + 1 if defect == "time_limit_one_step_late" else L
    ret, ln, trace = np.zeros(n), np.zeros(n, np.int32), np.zeros((n, L, ROW), F)
    env, obs = _oracle_at(case.seed, case.first, limit)
    for e in range(n):
        if defect == "episode_index_not_advanced":
            env, obs = _oracle_at(case.seed, case.first, limit)
        u0, u1 = da.uniforms(case.nseed, case.ctr + 2 * e * L, limit + 1)
        total, total32, t, prev, ended = 0.0, F(0.0), 0, None, False
        while not ended:
            seen = prev if (defect == "action_from_previous_obs" and prev is not None) else obs
            q = q_row32(params, seen, defect if defect in ("last_hidden2_dropped", "head_bias_of_action_3_dropped") else None)
            u1t = u1[t + 1] if defect == "u1_from_next_step" else u1[t]
            if defect == "argmax_takes_last_of_tie" and (case.deterministic or (case.family == "ddqn" and u0[t] < F(case.greedy))):
                act = _last_max(q)
            else:
                act = da.select(q, case.family, case.alpha, case.greedy, u0[t:t + 1], np.asarray([u1t], F), case.deterministic)
            _, rew, _, nxt, end = env.step(da.table_actions(act))
            ended = bool(end[0])
            if t < L:
                row = trace[e, t]
                row[:8], row[8:8 + A], row[16], row[17], row[18] = obs[0], q[0], F(act[0]), rew[0], F(ended)
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
            assert row[16] == np.trunc(row[16]) and row[16] >= 0, "%s: action %r is no index" % (where, row[16])
            _, rew, _, obs, end = env.step(da.table_actions(row[16:17]))
            ended = bool(end[0])
            assert _bits(row[17]) == _bits(rew[0]), "%s: reward %r, oracle %r" % (where, row[17], rew[0])
            assert _bits(row[18]) == _bits(F(ended)), "%s: ended %r, oracle %r" % (where, row[18], ended)
            assert _bits(row[19]) == 0, "%s: element 19 is %r" % (where, row[19])
            total, t = total + float(rew[0]), t + 1
        assert ln[e] == t, "%s episode %d: length %d, oracle %d" % (label, e, ln[e], t)
        assert ret[e] == total, "%s episode %d: return %r, float64 sum of the oracle's float32 rewards %r" % (label, e, ret[e], total)
        assert not _bits(trace[e, t:]).any(), "%s episode %d: rows past the end are not zero" % (label, e)


def played_rows(out):
    """The rows [steps, 20] of every step played, episode after episode."""
    trace = np.asarray(out["trace"], F)
    return np.concatenate([trace[e, :int(l)] for e, l in enumerate(out["len"])])


def q_reference(case, params, out):
    return ap.q_reference(case.q, params, played_rows(out)[:, :8])


def check_q(out, case, params, label="", table=None, ref=None):
    """(b) of the module docstring."""
    label = label or case.id
    rows = played_rows(out)
    A = case.acts
    assert not _bits(rows[:, 8 + A:16]).any(), "%s: q elements beyond action %d are not zero" % (label, A)
    want = q_row32(params, rows[:, :8])
    same = _bits(rows[:, 8:8 + A]) == _bits(want)
    at = np.argwhere(~same)
    assert same.all(), ("%s: %d of %d q elements differ from the float32 restatement of the kernel's summation order (first: step %d "
                        "action %d: %r, restated %r)" % (label, len(at), same.size, at[0][0], at[0][1], rows[at[0][0], 8 + at[0][1]], want[tuple(at[0])]))
    ap.compare(rows[:, 8:8 + A], q_reference(case, params, out) if ref is None else ref, "q1", label, table=table)


def call_uniforms(out, seed, ctr, max_ep_len):
    """(u0, u1) of every step played, episode after episode, for a call at (seed, ctr)."""
    u = [da.uniforms(seed, int(ctr) + 2 * e * int(max_ep_len), min(int(l), int(max_ep_len))) for e, l in enumerate(out["len"])]
    return np.concatenate([x[0] for x in u]), np.concatenate([x[1] for x in u])


def boundary_rows(out, case, seed=None, ctr=None):
    """SQN sampling: (float64 picks, rows whose u0 * total lies within 1e-5 relative of a float64 cumulative boundary)."""
    rows = played_rows(out)
    u0, _ = call_uniforms(out, case.nseed if seed is None else seed, case.ctr if ctr is None else ctr, case.max_ep_len)
    return da.sqn_boundaries64(rows[:, 8:8 + case.acts], case.alpha, u0)


def check_actions(out, case, seed=None, ctr=None, label=""):
    """(c) of the module docstring."""
    label = label or case.id
    seed, ctr = (case.nseed if seed is None else seed), (case.ctr if ctr is None else ctr)
    rows = played_rows(out)
    q, act = rows[:, 8:8 + case.acts], rows[:, 16]
    assert ((act == np.trunc(act)) & (act >= 0) & (act < case.acts)).all(), "%s: an action is not an index in [0, %d)" % (label, case.acts)
    u0, u1 = call_uniforms(out, seed, ctr, case.max_ep_len)
    if case.family == "sqn" and not case.deterministic:
        want, near = boundary_rows(out, case, seed, ctr)
        assert near.mean() <= MAX_EXCLUDED, "%s: %d of %d rows sit on a cumulative boundary (cap %g)" % (label, int(near.sum()), len(act), MAX_EXCLUDED)
        bad = (act != want) & ~near
    else:
        want = da.select(q, case.family, case.alpha, case.greedy, u0, u1, case.deterministic)
        bad = act != want
    assert not bad.any(), ("%s: %d of %d actions differ from the selection oracle on the trace's own q rows (first step %s: got %s, want %s)"
                           % (label, int(bad.sum()), len(act), np.nonzero(bad)[0][:1], act[bad][:1], want[bad][:1]))


def check_all(out, case, params, label="", table=None):
    check_env(out, case.seed, case.first, case.max_ep_len, label or case.id)
    check_q(out, case, params, label, table)
    check_actions(out, case, label=label)
