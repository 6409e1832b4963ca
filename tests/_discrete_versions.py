"""Helpers of tests/test_gpu_discrete_versions.py: the discrete rollout worker with a version store (RolloutDeviceDQN(adopt="episode")),
bias-coded Q networks whose Q row names the version an env acted on, the bookkeeping of what each env's own reference worker would hold
(algos/dqn/train.py:249-252: env.reset(), ps.pull, agent.set_weights — once per episode, for that env only), and restatements of what
tests/test_gpu_discrete_rollout.py keeps to itself (the checks collector, the action check, the C-level fused harness).

CODED VERSIONS.  Version v = zero kernels and hidden biases, head bias b3 = [v % 64, v // 64, 0, 0] for q1 — the acting network of both
families — and -1 everywhere for SQN's q2.  Every value is exactly representable and the Q row of an env is exactly its version's bias:
zero partials summed in any order, plus the bias."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _acting_parity as ap  # noqa: E402
import _discrete_acting as da  # noqa: E402

EPLEN, EPI = 10, 13          # csrc/env_device.h: per-env episode length / episode counter in the [32, n] state block
MAX_EXCLUDED = 0.01          # SQN sampling: share of rows that may sit on a cumulative boundary (tests/test_gpu_discrete_rollout.py)


def case(family, n, hidden=(64, 32), alpha=0.1, seed=5):
    return ap.QCase("%s-lander-%dx%d-n%d" % (family, hidden[0], hidden[1], n), family, 8, 4, hidden, n, alpha=alpha, seed=seed)


def coded(c, v):
    p = ap.q_params(c)
    for k in p:
        p[k] = np.zeros_like(p[k])
    p["main/q1/dense_2/bias"][:] = (v % 64, v // 64, 0, 0)
    if c.family == "sqn":
        p["main/q2/dense_2/bias"][:] = -1.0
    return p


def decode(q):
    """[n, 4] Q rows of coded versions -> [n] versions; asserts that they ARE coded rows."""
    q = np.asarray(q)
    assert (q[:, 2:] == 0).all() and (q[:, :2] == np.floor(q[:, :2])).all() and (q[:, :2] >= 0).all() and (q[:, 0] < 64).all(), q[:4]
    return (q[:, 0] + 64 * q[:, 1]).astype(int)


def make_opt(c, limit, adopt, start_steps=-1, cap=None, seed=3):
    class Opt:
        obs_dim, act_dim, hidden_size, gamma, lr, polyak, batch_size, alpha = c.obs, c.act, list(c.hid), 0.99, 1e-3, 0.995, c.batch, c.alpha
        num_envs, max_ep_len, variant, num_nodes, num_buffers, push_freq, a_l_ratio, save_dir = c.batch, limit, c.family, 1, 1, 50, 2, "."
        buffer_size = 4 * c.batch if cap is None else cap
    o = Opt()
    o.seed, o.start_steps, o.adopt = seed, start_steps, adopt
    return o


class Worker:
    """ParameterServer + ReplayBufferDQN + RolloutDeviceDQN of `c` (num_envs = c.batch) with the fused step's q mirror on."""

    def __init__(self, c, limit, params, adopt="episode", start_steps=-1, cap=None, stagger=True, seed=3):
        import distributed_drl_amd as ddrl
        from distributed_drl_amd.workers import RolloutDeviceDQN
        self.c, self.n, self.limit, self.keys = c, c.batch, limit, list(params.keys())
        self.opt = make_opt(c, limit, adopt, start_steps, cap, seed)
        self.ps = ddrl.ParameterServer(self.keys, list(params.values()))
        self.rb = ddrl.ReplayBufferDQN(self.opt, 0, seed=5)
        self.roll = RolloutDeviceDQN(self.ps, self.rb, self.opt)
        self.roll.q_out = torch.zeros(self.n, c.act, device="cuda")
        if stagger:               # stagger the time limits: episode ends in every step, env by env
            st = self.roll.env.get_state()
            st[EPLEN] = torch.arange(self.n, device="cuda").float() % limit
            self.roll.env.set_state(st)
        self.epi = self.roll.env.get_state()[EPI].cpu().numpy().copy()
        self.holds = np.zeros(self.n, int)     # the version env i's own worker_rollout_dqn holds (0: the initial pull)
        self.newest = 0                        # the version the server holds
        self.max_live = 1

    def push(self, v, params):
        self.newest = v
        self.ps.push(self.keys, list(params.values()))

    def ended_in_last_step(self):
        epi = self.roll.env.get_state()[EPI].cpu().numpy()
        ended, self.epi = epi > self.epi, epi.copy()
        return ended

    def step(self):
        """One vector step; -> the Q rows of the fused step (None in the random-action phase).  Afterwards `holds` is what every env's
        reference worker holds: an env whose episode ended in this step has pulled what the server held during it."""
        fused = self.roll.t > self.opt.start_steps
        self.roll.step()
        q = self.roll.q_out.cpu().numpy() if fused else None
        self.holds_before = self.holds.copy()
        self.holds[self.ended_in_last_step()] = self.newest
        self.max_live = max(self.max_live, len(set(self.holds.tolist())))
        return q


def sac_schedule(limit, steps, seed=5):
    """step -> version pushed right after it, on the schedule of the SAC test (tests/test_gpu_driver.py): a burst at the start, one every step
    for limit + 3 steps, nothing for more than `limit` steps, then at random."""
    rs = np.random.RandomState(seed)
    push_after, v = {}, 0
    for s in range(steps):
        if s < 12 or (20 <= s < 20 + limit + 3) or (s >= 20 + 2 * limit + 12 and rs.rand() < 0.4):
            v += 1
            push_after[s] = v
    return push_after


class Checks:
    """Collects failures and the measured q lines (tests/test_gpu_discrete_rollout.py::_Checks, restated)."""

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


def check_actions(ck, c, q_dev, act_dev, seed, ctr, greedy, label):
    """The device's actions against the NumPy selection on the device's own q rows and the oracle's uniforms: exact for Double-DQN; for SQN
    sampling a row may be excluded only if u0 * total lies within 1e-5 relative of a cumulative boundary recomputed in float64 from the
    device q row — at most MAX_EXCLUDED of the rows (tests/test_gpu_discrete_rollout.py::_check_actions, restated)."""
    q_dev, act_dev = np.asarray(q_dev, np.float32), np.asarray(act_dev)
    n = q_dev.shape[0]
    u0, u1 = da.uniforms(seed, ctr, n)
    ck.require(((act_dev == np.trunc(act_dev)) & (act_dev >= 0) & (act_dev < c.act)).all(), "%s: an action is not an index in [0, %d)" % (label, c.act))
    if c.family == "sqn":
        want, near = da.sqn_boundaries64(q_dev, c.alpha, u0)
        ck.require(near.mean() <= MAX_EXCLUDED, "%s: %d of %d rows sit on a cumulative boundary (cap %g)" % (label, int(near.sum()), n, MAX_EXCLUDED))
        bad = (act_dev != want) & ~near
    else:
        want = da.select(q_dev, c.family, c.alpha, greedy, u0, u1, False)
        bad = act_dev != want
    ck.require(not bad.any(), "%s: %d of %d actions differ from the selection oracle on the device's q rows (first row %s: got %s, want %s)"
               % (label, int(bad.sum()), n, np.nonzero(bad)[0][:1], act_dev[bad][:1], want[bad][:1]))


def q_actor(c, max_rows=None, params=None):
    from distributed_drl_amd import dqn

    class Opt:
        obs_dim, act_dim, hidden_size, gamma, lr, polyak, batch_size, seed, alpha = c.obs, c.act, list(c.hid), 0.99, 1e-3, 0.995, c.batch, c.seed, c.alpha
    actor = (dqn.ActorSQN if c.family == "sqn" else dqn.Actor)(Opt, "worker", max_rows=c.batch if max_rows is None else max_rows)
    params = ap.q_params(c) if params is None else params
    actor.set_weights(list(params.keys()), list(params.values()))
    return actor, params


class Fused:
    """n envs + an actor of `c` + a 1-D-acts ring, stepped through the C entry points, the three mirrors on
    (tests/test_gpu_discrete_rollout.py::_Fused, restated, with the time limits staggered)."""
    ENV_SEED, NOISE_SEED = 21, 0xC0FFEE

    def __init__(self, c, cap, n, limit, params=None, max_rows=None):
        from distributed_drl_amd import _lib
        from distributed_drl_amd.env import VecLunarLanderDiscrete
        from distributed_drl_amd.replay import ReplayBuffer

        class Ring1D(ReplayBuffer):
            _acts_1d = True
        self.lib, self._lib, self.c, self.n = _lib.load(), _lib, c, n
        self.actor, self.params = q_actor(c, max_rows=n if max_rows is None else max_rows, params=params)
        self.env = VecLunarLanderDiscrete(n, seed=self.ENV_SEED, max_ep_len=limit)
        st = self.env.get_state()
        st[EPLEN] = torch.arange(n, device="cuda").float() % limit
        self.env.set_state(st)
        self.rb = Ring1D(8, 1, cap)
        self.act, self.q, self.nxt = torch.zeros(n, device="cuda"), torch.zeros(n, c.act, device="cuda"), torch.zeros(n, 8, device="cuda")
        self.ctr = 0

    def begin(self):
        return self.lib.ddrl_rollout_begin_discrete(self.env._h, self.actor._h, self._lib.stream_ptr())

    def step(self, n_steps=1, mode=0, greedy=0.5):
        L = self._lib
        rc = self.lib.ddrl_rollout_step_discrete(self.env._h, self.actor._h, self.rb._h, n_steps, mode, greedy, self.NOISE_SEED, self.ctr, L.dptr(self.act),
                                                 L.dptr(self.q), L.dptr(self.nxt), L.stream_ptr())
        if rc == 0:
            self.ctr += 2 * self.n * n_steps
        return rc

    def snapshot(self, slots=False):
        r = self.rb.rings()
        out = dict(state=self.env.get_state().cpu().numpy(), counts=tuple(self.rb._counts()), nxt=self.nxt.cpu().numpy(), act=self.act.cpu().numpy(),
                   q=self.q.cpu().numpy(), **{k: v.cpu().numpy().copy() for k, v in r.items()})
        if slots:
            out["slots"] = self.actor.version_state()[0].cpu().numpy()
        return out


def same(a, b, what):
    assert set(a) == set(b)
    for k in a:
        if k == "counts":
            assert a[k] == b[k], "%s: ring counters %s != %s" % (what, a[k], b[k])
        else:
            np.testing.assert_array_equal(a[k], b[k], err_msg="%s: %s" % (what, k))
