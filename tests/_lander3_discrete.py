"""Helpers of tests/test_gpu_lander3_discrete_rollout.py and tests/test_lander3_discrete_rollout_cpu.py: the discrete rollout worker on the
ARTICULATED lander with its opt-in fused step (RolloutDeviceDQN, opt.fused_discrete_rollout_articulated), the cases of the Q-row /
selection test, and the CPU pre-check that keeps the SQN cases of that test off the cumulative boundaries.

SQN BOUNDARY CAP.  tests/_discrete_versions.check_actions lets MAX_EXCLUDED = 1 % of a step's rows sit within 1e-5 relative of a
cumulative boundary of the float64 inverse CDF: at n = 64 that is ZERO rows.  So the SQN cases below (weight seed, alpha, env seed,
time limit, number of steps) were chosen on the CPU: sqn_rows_near_a_boundary replays the run with the float32 Q oracle on
Lander3Oracle's observations and the oracle's uniforms, and counts the rows within a TEN TIMES WIDER margin, 1e-4 — wider than anything
the device's own q deviation (about 1e-6 relative) can move a row by.  The chosen cases have no such row in any checked step;
tests/test_lander3_discrete_rollout_cpu.py asserts that on every run."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _acting_parity as ap  # noqa: E402
import _discrete_acting as da  # noqa: E402
import _discrete_versions as dv  # noqa: E402

VIT, PIT = 8, 3              # the kernel's loops are run-time counts: the same code as at gym's 180 / 60
FLAG = "fused_discrete_rollout_articulated"
RINGS = ("obs1_buf", "obs2_buf", "acts_buf", "rews_buf", "done_buf")
NOISE_SEED = 0xC0FFEE

# ---- the Q-row / selection / fused-against-unfused test: (family, hidden, weight seed); n, env seed, time limit, steps, alpha for all
Q_N, Q_ENV_SEED, Q_LIMIT, Q_STEPS, Q_ALPHA, Q_GREEDY = 64, 3, 9, 12, 0.1, 0.5
Q_CASES = [("ddqn", (64, 48), 13), ("ddqn", (400, 300), 13), ("sqn", (64, 48), 13), ("sqn", (400, 300), 13)]


def case(family, n, hidden=(64, 48), alpha=0.1, seed=5):
    return ap.QCase("%s-lander3-%dx%d-n%d" % (family, hidden[0], hidden[1], n), family, 8, 4, hidden, n, alpha=alpha, seed=seed)


def q_case(family, hidden, seed):
    return case(family, Q_N, hidden=hidden, alpha=Q_ALPHA, seed=seed)


def make_opt(c, limit, adopt="step", start_steps=-1, cap=None, seed=3, vit=VIT, pit=PIT, flag=True, model="articulated"):
    o = dv.make_opt(c, limit, adopt, start_steps, cap, seed)
    if model != "simple":
        o.env_model, o.env_velocity_iterations, o.env_position_iterations = model, vit, pit
    if flag is not None:
        setattr(o, FLAG, flag)
    return o


def oracle(opt):
    from lander3_oracle import Lander3Oracle
    return Lander3Oracle(opt.num_envs, seed=opt.seed, max_ep_len=opt.max_ep_len, velocity_iterations=opt.env_velocity_iterations,
                         position_iterations=opt.env_position_iterations)


def sqn_rows_near_a_boundary(c, env_seed, limit, steps, margin=1e-4, noise_seed=NOISE_SEED):
    """The run of the Q-row test replayed on the CPU (see the module header): -> the number of rows, over all steps, whose u0 * total
    lies within `margin` relative of a cumulative boundary of the float64 inverse CDF of the float32 oracle's q rows."""
    from lander3_oracle import Lander3Oracle
    params = ap.q_params(c)
    ora = Lander3Oracle(c.batch, seed=env_seed, max_ep_len=limit, velocity_iterations=VIT, position_iterations=PIT)
    obs, near_rows = ora.obs(), 0
    for t in range(steps):
        q32 = ap.q_forward(c, params, obs, torch.float32)["q1"]
        u0, _ = da.uniforms(noise_seed, 2 * c.batch * t, c.batch)
        q64 = q32.astype(np.float64)
        cum = np.cumsum(np.exp((q64 - q64.max(axis=1, keepdims=True)) / float(np.float32(c.alpha))), axis=1)
        tt = u0.astype(np.float64) * cum[:, -1]
        near_rows += int((np.abs(tt[:, None] - cum) <= margin * np.abs(cum)).any(axis=1).sum())
        obs = ora.step(da.table_actions(da.select_sqn(q32, c.alpha, u0)))[3]
    return near_rows


class Worker:
    """ParameterServer + ReplayBufferDQN + RolloutDeviceDQN of `c` (num_envs = c.batch) on the articulated lander, the q mirror's copy
    on.  fused=True asserts that the worker HAS decided for the fused pair (a silent fallback fails here)."""

    def __init__(self, c, limit, params, fused=True, rb=None, **kw):
        import distributed_drl_amd as ddrl
        from distributed_drl_amd.workers import RolloutDeviceDQN
        self.c, self.n, self.limit, self.keys = c, c.batch, limit, list(params.keys())
        self.opt = make_opt(c, limit, **kw)
        self.ps = ddrl.ParameterServer(self.keys, list(params.values()))
        self.rb = ddrl.ReplayBufferDQN(self.opt, 0, seed=5) if rb is None else rb
        self.cap = self.rb.max_size
        self.roll = RolloutDeviceDQN(self.ps, self.rb, self.opt)
        self.roll.q_out = torch.zeros(self.n, c.act, device="cuda")
        if fused is not None:
            assert self.roll._fused_ready() is fused and self.roll._fused is fused
        self.newest = 0

    def stagger(self):
        """Stagger the time limits through set_state: episode ends in every step, env by env."""
        st = self.roll.env.get_state()
        st[dv.EPLEN] = torch.arange(self.n, device="cuda").float() % self.limit
        self.roll.env.set_state(st)
        self.epi = self.roll.env.get_state()[dv.EPI].cpu().numpy().copy()
        self.holds = np.zeros(self.n, int)     # the version env i's own worker_rollout_dqn holds (0: the initial pull)
        self.max_live = 1

    def push(self, v, params):
        self.newest = v
        self.ps.push(self.keys, list(params.values()))

    def fused_step(self, n_steps=1):
        self.roll.step(n_steps)
        assert self.roll._fused is True and self.roll._fused_live, "the step did not take the fused launch"

    def versioned_step(self):
        """One fused step of a staggered worker; -> (the step's Q rows, what every env's reference worker held BEFORE the step).
        Afterwards `holds` is what they hold now: an env whose episode ended in this step has pulled what the server held during it."""
        self.fused_step()
        q, before = self.roll.q_out.cpu().numpy(), self.holds.copy()
        epi = self.roll.env.get_state()[dv.EPI].cpu().numpy()
        self.holds[epi > self.epi] = self.newest
        self.epi = epi.copy()
        self.max_live = max(self.max_live, len(set(self.holds.tolist())))
        return q, before

    def snapshot(self, slots=False):
        roll = self.roll
        act, q, nxt = roll.env.rollout_mirrors()
        out = dict(state=roll.env.get_state().cpu().numpy(), counts=tuple(self.rb._counts()), obs=roll.env.obs.cpu().numpy(),
                   act=roll.act.cpu().numpy(), q=roll.q_out.cpu().numpy(), m_act=act.cpu().numpy(), m_q=q.cpu().numpy(), m_nxt=nxt.cpu().numpy(),
                   **{k: v.cpu().numpy().copy() for k, v in self.rb.rings().items()})
        if slots:
            out["slots"] = roll.actor.version_state()[0].cpu().numpy()
        return out


def lockstep(w, ora, steps, t0=0, fused_from=0):
    """`steps` vector steps of the worker beside the oracle, which is fed the worker's own actions through the action table: the next
    observation and the step's ring rows bit for bit after every step.  -> (done rows, ended rows) of the steps from `fused_from` on."""
    roll, n, cap = w.roll, w.n, w.cap
    done, ended = [], []
    for t in range(t0, t0 + steps):
        obs = roll.env.obs.cpu().numpy().copy()
        np.testing.assert_array_equal(obs, ora.obs(), err_msg="obs before step %d" % t)
        if t >= fused_from:
            w.fused_step()
        else:
            roll.step()
            assert not roll._fused_live
        act = roll.act.cpu().numpy().copy()
        o2, r, d, nxt, end = ora.step(da.table_actions(act))
        np.testing.assert_array_equal(roll.env.obs.cpu().numpy(), nxt, err_msg="next obs, step %d" % t)
        rings = w.rb.rings()
        rows = (t * n + np.arange(n)) % cap
        for k, want in zip(RINGS, (obs, o2, act, r, d)):
            got = rings[k].cpu().numpy()[rows].reshape(np.asarray(want).shape)
            np.testing.assert_array_equal(got, np.asarray(want, np.float32), err_msg="%s step %d" % (k, t))
        if t >= fused_from:
            done.append(np.asarray(d).copy())
            ended.append(np.asarray(end).copy())
    return np.array(done), np.array(ended)


def check_end(w, ora, total_steps):
    """Env state, episode statistics, ring counters and cursor against the oracle at the end of a run; -> episodes ended."""
    np.testing.assert_array_equal(w.roll.env.get_state().cpu().numpy(), ora.S)
    ge, gr, gl = w.roll.env.stats()
    we, wr, wl = ora.stats()
    assert (ge, gl) == (we, wl)
    assert abs(gr - wr) <= 1e-9 * max(1.0, abs(wr))
    stored = total_steps * w.n
    assert tuple(w.rb._counts())[:3] == (stored % w.cap, min(stored, w.cap), stored)
    assert w.rb.ptr == stored % w.cap
    return ge
