"""The discrete actors' device path: ddrl_env_step_discrete, ddrl_dqn_act (dqn.Actor / ActorSQN.get_actions), the fused discrete rollout
step (ddrl_rollout_begin_discrete / ddrl_rollout_step_discrete) and RolloutDeviceDQN under ActorLearnerLoop.

REFERENCES  the lander: oracle/env_oracle.LanderOracle fed the table-mapped actions, bit for bit; the ring: oracle/replay_oracle, bit
            for bit; the Q rows: the float64 forward of tests/_acting_parity.py under its compare(..., "q1") rule (twice the float32
            oracle ensemble's own deviation under permuted summation orders); the actions: tests/_discrete_acting.py applied to the
            DEVICE's own q rows and the oracle's uniforms — exactly for Double-DQN and SQN deterministic; for SQN sampling a row may be
            excluded only if u0 * total lies within 1e-5 relative of a cumulative boundary recomputed in float64 from the device q row
            (at most 1 % of the rows: asserted; with <= 7 boundaries per row the expected share is below 2e-4).
DDRL_ACTING_TABLE=<file>: append the measured q lines to that file (profiles/acting_parity_observed.txt holds one such run)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _acting_parity as ap  # noqa: E402
import _discrete_acting as da  # noqa: E402

from oracle import dqn_oracle as do  # noqa: E402
from oracle import sac1_oracle as so  # noqa: E402

pytestmark = pytest.mark.gpu

LANDER_DDQN = ap.QCase("ddqn-lander-400x300", "ddqn", 8, 4, (400, 300), 64, seed=12)      # the reference's default widths: ragged column tiles
LANDER_SQN = ap.QCase("sqn-lander-64x32", "sqn", 8, 4, (64, 32), 64, alpha=0.1, seed=13)
ACT_CASES = [c for c in ap.Q_CASES if c.id in ("ddqn-ragged", "sqn-aligned", "ddqn-wide-1028")] + [LANDER_DDQN, LANDER_SQN]
MAX_EXCLUDED = 0.01


@pytest.fixture(scope="module")
def ddrl():
    import distributed_drl_amd as d
    d._lib.require_gpu()
    return d


class _Checks:
    def __init__(self):
        self.table, self.bad = [], []

    def compare(self, got, ref, kind, label):
        got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
        try:
            ap.compare(got, ref, kind, label, False, self.table)
        except AssertionError as e:
            self.bad.append(str(e))

    def require(self, ok, what):
        if not ok:
            self.bad.append(what)

    def finish(self):
        lines = ap.format_table(self.table)
        path = os.environ.get("DDRL_ACTING_TABLE")
        if path and lines:
            with open(path, "a") as f:
                f.write("\n".join(lines) + "\n")
        assert not self.bad, "\n".join(self.bad + ["measured:"] + lines)


def _q_actor(case, max_rows=None, params=None):
    from distributed_drl_amd import dqn

    class Opt:
        obs_dim, act_dim, hidden_size, gamma, lr, polyak, batch_size, seed, alpha = case.obs, case.act, list(case.hid), 0.99, 1e-3, 0.995, case.batch, case.seed, case.alpha
    actor = (dqn.ActorSQN if case.family == "sqn" else dqn.Actor)(Opt, "worker", max_rows=case.batch if max_rows is None else max_rows)
    params = ap.q_params(case) if params is None else params
    actor.set_weights(list(params.keys()), list(params.values()))
    return actor, params


def _check_actions(ck, case, q_dev, act_dev, seed, ctr, greedy, deterministic, label):
    """2(b): the device's actions against the NumPy selection on the device's own q rows and the oracle's uniforms."""
    q_dev, act_dev = np.asarray(q_dev, np.float32), np.asarray(act_dev)
    n = q_dev.shape[0]
    u0, u1 = da.uniforms(seed, ctr, n)
    ck.require(((act_dev == np.trunc(act_dev)) & (act_dev >= 0) & (act_dev < case.act)).all(), "%s: an action is not an index in [0, %d)" % (label, case.act))
    if case.family == "sqn" and not deterministic:
        want, near = da.sqn_boundaries64(q_dev, case.alpha, u0)
        ck.require(near.mean() <= MAX_EXCLUDED, "%s: %d of %d rows sit on a cumulative boundary (cap %g)" % (label, int(near.sum()), n, MAX_EXCLUDED))
        bad = (act_dev != want) & ~near
    else:
        want = da.select(q_dev, case.family, case.alpha, greedy, u0, u1, deterministic)
        bad = act_dev != want
    ck.require(not bad.any(), "%s: %d of %d actions differ from the selection oracle on the device's q rows (first row %s: got %s, want %s)"
               % (label, int(bad.sum()), n, np.nonzero(bad)[0][:1], act_dev[bad][:1], want[bad][:1]))
    return u0


# ---- 1. ddrl_env_step_discrete ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,seed,max_len", [(1, 3, 1000), (64, 1, 40), (300, 7, 1000)])
def test_env_step_discrete_bit_exact_vs_oracle(ddrl, n, seed, max_len):
    from distributed_drl_amd.env import VecLunarLanderDiscrete
    from oracle.env_oracle import LanderOracle
    env, ora = VecLunarLanderDiscrete(n, seed=seed, max_ep_len=max_len), LanderOracle(n, seed=seed, max_ep_len=max_len)
    np.testing.assert_array_equal(env.obs.cpu().numpy(), ora.obs())
    rs = np.random.RandomState(seed)
    values = np.array([0, 1, 2, 3, -1, 7], np.float32)
    seen, n_ended = set(), 0
    for t in range(200):
        idx = values[rs.randint(0, len(values), n)]
        seen |= set(idx.tolist())
        g = [x.cpu().numpy() for x in env.step(torch.from_numpy(idx).cuda())]
        w = ora.step(da.table_actions(idx))
        for name, gv, wv in zip(("obs2", "rew", "done", "next_obs", "ended"), g, w):
            np.testing.assert_array_equal(gv, wv, err_msg="%s at step %d" % (name, t))
        n_ended += int(w[4].sum())
    assert seen == set(values.tolist())
    np.testing.assert_array_equal(env.get_state().cpu().numpy(), ora.S)
    ge, gr, gl = env.stats()
    we, wr, wl = ora.stats()
    assert (ge, gl) == (we, wl) and ge == n_ended
    assert abs(gr - wr) <= 1e-9 * max(1.0, abs(wr))
    if max_len == 40:
        assert n_ended > 0


def test_discrete_facade_and_sampler(ddrl):
    from distributed_drl_amd import env as E
    from oracle import noise_oracle as no
    e = E.make("LunarLander-v2", seed=2, max_ep_len=30)
    assert e.action_space.n == 4 and e.reset().shape == (8,)
    assert 0 <= e.action_space.sample() <= 3
    for k in range(40):
        o2, r, d, _ = e.step(k % 4)
        if d:
            break
    assert d and o2.shape == (8,)
    assert type(E.make("LunarLanderContinuous-v2")).__name__ == "LunarLander"
    v = E.VecLunarLanderDiscrete(100, seed=9)
    assert v.act_dim == 4
    for _ in range(2):
        ctr = v._sample_ctr
        np.testing.assert_array_equal(v.sample_actions().cpu().numpy(), np.floor(no.uniform_fill(100, 0.0, 4.0, 9 ^ 0x5EED5EED, ctr)))


# ---- 2. get_actions ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ACT_CASES, ids=repr)
def test_get_actions_q_rows_and_selection(ddrl, case):
    ck = _Checks()
    actor, params = _q_actor(case)
    obs = ap.q_inputs(case)
    ref = ap.q_reference(case, params, obs)
    path = "wide" if case.obs >= 1024 else ("mfma" if (case.hid[0] % 4 == 0 and case.hid[1] % 4 == 0 and case.obs + (case.act + 1) // 2 <= 12) else "generic")
    sqn = case.family == "sqn"
    for n in [k for k in (case.batch, 1, 32, 37) if k <= case.batch]:      # the short calls come after a full one
        for greedy, det in ((0.5, False), (0.97, False)) + (((0.97, True),) if sqn else ()):
            q = torch.full((n, case.act), float("nan"), device="cuda")
            seed, ctr = actor._noise_seed, actor._noise_ctr
            actor.greedy_prob = greedy
            act = actor.get_actions(obs[:n], q_out=q, deterministic=det)
            assert actor._noise_ctr == ctr + 2 * n and act.shape == (n,)
            label = "%s get_actions (%s) n=%d greedy=%g%s" % (case.id, path, n, greedy, " deterministic" if det else "")
            if greedy == 0.5 and not det:
                ck.compare(q, ref.rows(slice(0, n)), "q1", label)
            u0 = _check_actions(ck, case, q.cpu().numpy(), act.cpu().numpy(), seed, ctr, greedy, det, label)
            if not sqn and greedy == 0.5 and n >= 32:
                ck.require((u0 < 0.5).any() and (u0 >= 0.5).any(), "%s: one branch of the coin flip never occurred" % label)
    # out= is written in place, and a given (seed, counter) gives the call again
    n = min(case.batch, 32)
    out = torch.empty(n, device="cuda")
    actor._noise_ctr = 1000
    a1 = actor.get_actions(obs[:n], out=out).clone()
    actor._noise_ctr = 1000
    assert actor.get_actions(obs[:n]).equal(a1) and out.equal(a1)
    ck.finish()


@pytest.mark.parametrize("case", [LANDER_DDQN, LANDER_SQN], ids=repr)
def test_copied_columns_return_the_first_index(ddrl, case):
    """A network whose last-layer columns 1 and 2 are copies, bias included: index 1 wherever those columns hold the row maximum."""
    params = ap.q_params(case)
    for q in case.nets:
        k, b = params["main/%s/dense_2/kernel" % q].copy(), params["main/%s/dense_2/bias" % q].copy()
        k[:, 2], b[1] = k[:, 1], b[1] + 0.3
        b[2] = b[1]
        params["main/%s/dense_2/kernel" % q], params["main/%s/dense_2/bias" % q] = k, b
    actor, _ = _q_actor(case, params=params)
    obs = ap.q_inputs(case)
    q = torch.empty(case.batch, case.act, device="cuda")
    act = actor.get_actions(obs, q_out=q, deterministic=True).cpu().numpy()
    q = q.cpu().numpy()
    np.testing.assert_array_equal(q[:, 1], q[:, 2])
    top = q[:, 1] >= q.max(axis=1)
    assert top.sum() >= 8, top.sum()
    assert (act[top] == 1).all()
    np.testing.assert_array_equal(act, np.argmax(q, axis=1))


# ---- 3. the fused step ---------------------------------------------------------------------------------------------------------------------
N_ENVS, EP_LEN, ENV_SEED, NOISE_SEED = 64, 40, 21, 0xC0FFEE
PRE_ROLL = 33        # unfused steps in front of the 12 fused calls of the oracle runs


def _ring(cap, act_dim=1):
    from distributed_drl_amd.replay import ReplayBuffer

    class Ring1D(ReplayBuffer):
        _acts_1d = True
    return Ring1D(8, 1, cap) if act_dim == 1 else ReplayBuffer(8, act_dim, cap)


class _Fused:
    """n envs + an actor of `case` + a ring of `cap` rows, with the three mirrors on."""

    def __init__(self, case, cap, n=N_ENVS, ring=None, params=None):
        from distributed_drl_amd import _lib
        from distributed_drl_amd.env import VecLunarLanderDiscrete
        self.lib, self._lib, self.case, self.n = _lib.load(), _lib, case, n
        self.actor, self.params = _q_actor(case, max_rows=n, params=params)
        self.env = VecLunarLanderDiscrete(n, seed=ENV_SEED, max_ep_len=EP_LEN)
        self.rb = _ring(cap) if ring is None else ring
        self.act, self.q, self.nxt = torch.zeros(n, device="cuda"), torch.zeros(n, case.act, device="cuda"), torch.zeros(n, 8, device="cuda")
        self.ctr = 0

    def begin(self):
        return self.lib.ddrl_rollout_begin_discrete(self.env._h, self.actor._h, self._lib.stream_ptr())

    def step(self, n_steps=1, mode=0, greedy=0.5):
        L = self._lib
        rc = self.lib.ddrl_rollout_step_discrete(self.env._h, self.actor._h, self.rb._h, n_steps, mode, greedy, NOISE_SEED, self.ctr, L.dptr(self.act),
                                                 L.dptr(self.q), L.dptr(self.nxt), L.stream_ptr())
        if rc == 0:
            self.ctr += 2 * self.n * n_steps
        return rc

    def snapshot(self):
        r = self.rb.rings()
        return dict(state=self.env.get_state().cpu().numpy(), counts=tuple(self.rb._counts()), nxt=self.nxt.cpu().numpy(), act=self.act.cpu().numpy(),
                    q=self.q.cpu().numpy(), **{k: v.cpu().numpy().copy() for k, v in r.items()})


def _same(a, b, what, skip=()):
    for k in a:
        if k in skip:
            continue
        if k == "counts":
            assert a[k] == b[k], "%s: ring counters %s != %s" % (what, a[k], b[k])
        else:
            np.testing.assert_array_equal(a[k], b[k], err_msg="%s: %s" % (what, k))


def _run_against_oracles(case, cap, calls=12, check_q=True, new_params_at=None):
    from oracle.env_oracle import LanderOracle
    from oracle.replay_oracle import ReplayBufferOracle
    ck = _Checks()
    f = _Fused(case, cap)
    ora, rbo = LanderOracle(N_ENVS, seed=ENV_SEED, max_ep_len=EP_LEN), ReplayBufferOracle(8, 1, cap, acts_1d=True)
    rs = np.random.RandomState(1)
    for _ in range(PRE_ROLL):        # episodes EP_LEN - PRE_ROLL steps from their time limit: the fused calls see the resets
        idx = rs.randint(0, 4, N_ENVS).astype(np.float32)
        f.env.step(torch.from_numpy(idx).cuda())
        ora.step(da.table_actions(idx))
    f.env.stats()
    ora.episodes, ora.ret_sum, ora.len_sum = 0, 0.0, 0
    assert f.begin() == 0, f.lib.ddrl_last_error()
    o, params, n_ended = ora.obs(), f.params, 0
    for t in range(calls):
        if new_params_at == t:
            old, params = params, ap.q_params(case, version=1)
            f.actor.set_weights(list(params.keys()), list(params.values()))
        ctr = f.ctr
        assert f.step() == 0, f.lib.ddrl_last_error()
        g = f.snapshot()
        label = "%s fused cap %d call %d" % (case.id, cap, t)
        if check_q or new_params_at == t:
            ck.compare(g["q"], ap.q_reference(case, params, o), "q1", label)
        if new_params_at == t:      # ... and not the old parameters' reference
            with pytest.raises(AssertionError):
                ap.compare(g["q"], ap.q_reference(case, old, o), "q1", label + " (old parameters)")
        _check_actions(ck, case, g["q"], g["act"], NOISE_SEED, ctr, 0.5, False, label)
        o2, r, d, nxt, ended = ora.step(da.table_actions(g["act"]))
        rbo.store_batch(o, g["act"], r, o2, d)
        n_ended += int(ended.sum())
        rows = np.arange(rbo.size)
        for k, w in (("obs1_buf", rbo.obs1_buf), ("obs2_buf", rbo.obs2_buf), ("acts_buf", rbo.acts_buf), ("rews_buf", rbo.rews_buf), ("done_buf", rbo.done_buf)):
            np.testing.assert_array_equal(g[k][rows], w[rows], err_msg="%s: %s" % (label, k))
        if cap >= N_ENVS:             # the stored action column is the action mirror
            np.testing.assert_array_equal(g["acts_buf"][(rbo.ptr - N_ENVS + np.arange(N_ENVS)) % cap], g["act"], err_msg=label)
        np.testing.assert_array_equal(g["nxt"], nxt, err_msg=label + ": next-observation mirror")
        np.testing.assert_array_equal(g["state"], ora.S, err_msg=label + ": env state block")
        assert g["counts"][:3] == (rbo.ptr, rbo.size, rbo.steps), (label, g["counts"], (rbo.ptr, rbo.size, rbo.steps))
        o = nxt
    assert (n_ended > 0 or calls < EP_LEN - PRE_ROLL) and len(set(f.rb.rings()["acts_buf"].cpu().numpy()[:min(cap, 700)].tolist())) == 4
    ge, _, gl = f.env.stats()
    assert (ge, gl) == (ora.episodes, ora.len_sum)
    ck.finish()


@pytest.mark.parametrize("case", [LANDER_DDQN, LANDER_SQN], ids=repr)
def test_fused_step_against_the_oracles(ddrl, case):
    _run_against_oracles(case, 1000)


@pytest.mark.parametrize("case", [LANDER_DDQN, LANDER_SQN], ids=repr)
@pytest.mark.parametrize("cap", [100, 48])
def test_fused_step_wraps_and_skips_overwritten_rows(ddrl, case, cap):
    _run_against_oracles(case, cap, check_q=False)


@pytest.mark.parametrize("case", [LANDER_DDQN, LANDER_SQN], ids=repr)
def test_fused_step_sees_new_weights(ddrl, case):
    _run_against_oracles(case, 1000, calls=4, check_q=False, new_params_at=2)


@pytest.mark.parametrize("case", [LANDER_DDQN, LANDER_SQN], ids=repr)
def test_four_steps_in_one_call_equal_four_calls(ddrl, case):
    a, b = _Fused(case, 1000), _Fused(case, 1000)
    assert a.begin() == 0 and b.begin() == 0
    assert a.step(4) == 0
    for _ in range(4):
        assert b.step(1) == 0
    assert a.ctr == b.ctr
    _same(a.snapshot(), b.snapshot(), "n_steps = 4 against 4 x n_steps = 1")
    assert a.step(1) == 0 and b.step(1) == 0          # the observation buffers inside the handles: the next step acts on them
    _same(a.snapshot(), b.snapshot(), "the step after")


@pytest.mark.parametrize("case", [LANDER_DDQN, LANDER_SQN], ids=repr)
def test_fused_equals_unfused(ddrl, case):
    a, b = _Fused(case, 100), _Fused(case, 100)
    assert a.begin() == 0
    b.actor._noise_seed, b.actor._noise_ctr, b.actor.greedy_prob = NOISE_SEED, 0, 0.5
    for t in range(6):
        assert a.step() == 0
        o = b.env.obs.clone()
        b.actor.get_actions(o, out=b.act, q_out=b.q)
        o2, r, d, nxt, _ = b.env.step(b.act)
        b.rb.store_batch(o, b.act, r, o2, d)
        b.nxt.copy_(nxt)
        _same(a.snapshot(), b.snapshot(), "fused against get_actions + env.step + store_batch, step %d" % t)
    assert b.actor._noise_ctr == a.ctr


def test_fused_step_refusals(ddrl):
    from distributed_drl_amd import _lib
    case = LANDER_DDQN
    # n = 48: outside the envelope
    f = _Fused(case, 1000, n=48)
    before = f.snapshot()
    assert f.begin() == _lib.DDRL_ERR_UNSUPPORTED and b"32" in f.lib.ddrl_last_error()
    assert f.step() == _lib.DDRL_ERR_UNSUPPORTED
    _same(before, f.snapshot(), "refused n = 48")
    # a ring with 2-wide acts: another layout
    f = _Fused(case, 1000, ring=_ring(1000, act_dim=2))
    assert f.begin() == 0
    before = f.snapshot()
    assert f.step() == _lib.DDRL_ERR_BAD_ARG
    _same(before, f.snapshot(), "refused ring layout")
    assert f.rb._counts()[2] == 0
    # hidden sizes outside the direct-operand limits: the reason names them
    g = _Fused(ap.QCase("ddqn-h50", "ddqn", 8, 4, (50, 34), 64), 1000)
    assert g.begin() == _lib.DDRL_ERR_UNSUPPORTED and b"hidden" in g.lib.ddrl_last_error()


# ---- 4. acting does not disturb learning ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [LANDER_DDQN, LANDER_SQN] + [c for c in ap.Q_CASES if c.id == "ddqn-wide-1028"], ids=repr)
def test_get_actions_between_updates_leaves_the_learner_unchanged(ddrl, case):
    from distributed_drl_amd import _lib
    cfg = ap.q_cfg(case)
    batches = [do.synthetic_batch(cfg, 500 + i) for i in range(3)]
    obs = ap.q_inputs(case, 1)
    out, acts = [], []
    for acting in (False, True):
        learner, _ = _q_actor(case)
        learner.train(batches[0], 0)
        if acting:
            acts.append(learner.get_actions(obs[:case.batch // 2]).clone())
            learner.get_actions(obs[:1], deterministic=True)
        learner.train(batches[1], 1)
        if acting:
            q = torch.empty(case.batch, case.act, device="cuda")
            learner.get_actions(obs, q_out=q)
            # ... and acts on the parameters the updates have left: the q rows are those of ddrl_dqn_q on the same handle
            ap.compare(q.cpu().numpy(), ap.q_reference(case, _params_of(learner, case), obs), "q1", "%s get_actions after two updates" % case.id)
        learner.train(batches[2], 2)
        out.append([learner.export(c).clone() for c in (_lib.SAC1_MAIN, _lib.SAC1_TARGET, _lib.SAC1_ADAM_M, _lib.SAC1_ADAM_V)])
    for name, a, b in zip(("main", "target", "m", "v"), *out):
        assert torch.equal(a, b), "%s: %s differs when the learner acts between its updates (max |diff| %.3e)" % (case.id, name, (a - b).abs().max().item())
    assert not torch.equal(out[0][0], torch.from_numpy(so.flatten(ap.q_params(case))).cuda())


def _params_of(learner, case):
    keys, vals = learner.get_weights()
    p = ap.q_params(case)
    return type(p)((k, np.asarray(v, np.float32)) for k, v in zip(keys, vals))


# ---- 5. wiring -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["ddqn", "sqn"])
def test_rollout_device_dqn_under_the_actor_learner_loop(ddrl, family):
    from distributed_drl_amd import dqn
    from distributed_drl_amd.ps import ParameterServer
    from distributed_drl_amd.replay import ReplayBufferDQN
    from distributed_drl_amd.workers import ActorLearnerLoop, RolloutDeviceDQN, TrainDeviceDQN

    class Opt:
        obs_dim, act_dim, hidden_size, gamma, lr, polyak, batch_size, seed, alpha = 8, 4, [64, 48], 0.99, 1e-3, 0.995, 64, 3, 0.1
        num_envs, max_ep_len, start_steps, a_l_ratio, num_nodes, num_buffers, push_freq, buffer_size, variant = 64, 40, 128, 2, 1, 1, 50, 4096, family
    opt = Opt()
    L = dqn.LearnerSQN if family == "sqn" else dqn.Learner
    seed_learner = L(opt)
    ps = ParameterServer(*seed_learner.get_weights())
    rb = ReplayBufferDQN(opt, 0, seed=5)
    rollout = RolloutDeviceDQN(ps, rb, opt)
    assert isinstance(rollout.actor, dqn.ActorSQN if family == "sqn" else dqn.Actor)
    trainer = TrainDeviceDQN([ps], [[rb]], opt, make_agent=lambda o_: L(o_, job="learner"), rng=np.random.RandomState(0))
    loop = ActorLearnerLoop(rollout, trainer, opt)
    rollout.auto_pull = False
    obs = torch.from_numpy(ap.q_inputs(LANDER_SQN)).cuda()
    q0 = torch.empty(64, 4, device="cuda")
    rollout.actor.get_actions(obs, q_out=q0)
    loop.run(30)
    torch.cuda.synchronize()
    samples, steps, size = rb.get_counts()
    assert steps == 30 * 64 and size == 30 * 64 and rollout.t == 30 * 64
    assert rollout._fused is True                                     # the policy phase took the fused launch pair
    want = 0
    for k in range(1, 31):
        want += max(0, (64 * k) // 2 - want) if 64 * k > 128 else 0
    assert samples == want == loop.sample_times and want > 0
    assert np.isfinite(trainer.agent.loss.item())
    rb.check()
    trainer.agent.export()                                            # (a poisoned learner refuses)
    acts = rb.rings()["acts_buf"][:steps].cpu().numpy()
    assert set(acts.tolist()) == {0.0, 1.0, 2.0, 3.0}
    # a push reaches the rollout's actor
    q_same = torch.empty(64, 4, device="cuda")
    rollout.actor.get_actions(obs, q_out=q_same)
    assert torch.equal(q0, q_same)
    assert rollout.pull() is True
    q1 = torch.empty(64, 4, device="cuda")
    rollout.actor.get_actions(obs, q_out=q1)
    assert not torch.equal(q0, q1)
    keys, vals = trainer.agent.get_weights()
    if want % opt.push_freq == 0:
        for k, v in zip(keys, vals):
            np.testing.assert_array_equal(dict(zip(*rollout.actor.get_weights()))[k], v)
