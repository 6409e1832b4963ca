"""workers.RolloutDeviceNStep on the BIPEDAL WALKER (opt.env_model = "walker"): the n-step driver's worker on the env the reference runs
it on.  32 envs, Ln 4, 8 / 3 iterations, limit_steps 6.  The worker is compared bit for bit, after every vector step of the random
phase and of the policy phase, with a twin driven by hand through the public objects (sample_actions / Actor.get_actions,
VecBipedalWalker.step_wrapped_walker, WindowQueue.push / begin, ReplayBufferNStep.store_masked) from the same seeds and the same noise
counter; it is unfused and without a version store, adopts a pushed policy as a whole vector after its next step, feeds a learner on
the generic launch path, and checks its rings before it allocates anything."""
import gc
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

N, LN, VIT, PIT, LIMIT, START = 32, 4, 8, 3, 6, 5


@pytest.fixture(scope="module")
def ddrl():
    import distributed_drl_amd as d
    d._lib.require_gpu()
    torch.cuda.set_device(0)
    return d


def _opt(obs_dim=24, act_dim=4):
    from distributed_drl_amd.agent import HyperParameters
    opt = HyperParameters(obs_dim=obs_dim, act_dim=act_dim)
    opt.hidden_sizes = (64, 48)
    opt.num_envs, opt.seed, opt.Ln, opt.save_freq, opt.start_steps = N, 3, LN, 1, START
    opt.max_ep_len, opt.action_repeat = 12, 2                    # limit_steps = ceil(12 / 2) = 6
    opt.buffer_size, opt.batch_size, opt.num_buffers = 150, 8, 1
    opt.obs_noise, opt.act_noise, opt.reward_scale = 0.01, 0.3, 5
    opt.env_model, opt.env_velocity_iterations, opt.env_position_iterations = "walker", VIT, PIT
    return opt


def _perturbed(vals, v):
    rs = np.random.RandomState(100 + v)
    return [(w + (0.3 * rs.standard_normal(w.shape)).astype(np.float32) * (0.2 if w.ndim == 2 else 1.0)) for w in vals]


class _HandTwin:
    """sac_ray.py:208-262 for N envs through the public objects, one call per statement of RolloutDeviceNStep._step_once's unfused
    sequence — written out here, not taken from the worker."""

    def __init__(self, ddrl, ps, opt):
        from distributed_drl_amd.agent import Actor
        from distributed_drl_amd.env import VecBipedalWalker
        from distributed_drl_amd.workers import WindowQueue
        self.opt, self.ps = opt, ps
        self.rb = ddrl.ReplayBufferNStep(opt)
        self.env = VecBipedalWalker(N, seed=opt.seed, max_ep_len=1 << 23, velocity_iterations=VIT, position_iterations=PIT)
        self.actor = Actor(opt, job="worker", max_rows=N, index=0)
        self.keys = list(self.actor.keys)
        self.actor.set_weights(self.keys, ps.pull_device(self.keys))
        self.version = ps.version
        self.winq = WindowQueue(N, LN, 24, 4, 1)
        self.winq.begin(self.env.obs)
        self.o = torch.empty_like(self.env.obs)
        self.act = torch.empty(N, 4, device="cuda")
        self.filling = 0

    def step(self):
        env, opt = self.env, self.opt
        self.o.copy_(env.obs)
        if self.filling > opt.start_steps:
            self.actor.get_actions(self.o, out=self.act)
        else:
            env.sample_actions(out=self.act)
            self.filling += 1
        o2, r, d, nxt, ended = env.step_wrapped_walker(self.act, opt.act_noise, opt.obs_noise, opt.reward_scale, 3, LIMIT)
        ready = self.winq.push(o2, self.act, r, d)
        self.rb.store_masked(*self.winq.arrays, ready)
        self.winq.begin(nxt, ended)
        if self.ps.version != self.version:
            self.version = self.ps.version
            self.actor.set_weights(self.keys, self.ps.pull_device(self.keys))


def _snap(w, rb):
    c = lambda t: t.detach().cpu().numpy().copy()
    s = dict(act=c(w.act), obs=c(w.env.obs), ended=c(w.env.ended), state=c(w.env.get_state()))
    for k, a in zip("oard", w.winq.arrays):
        s["q" + k] = c(a)
    for k, a in rb.rings().items():
        s[k] = c(a)
    s["counts"] = np.array(rb._counts()[:3])   # ptr, size, steps
    return s


def test_the_worker_equals_a_twin_driven_by_hand_and_feeds_a_learner(ddrl):
    from distributed_drl_amd.agent import Learner
    opt = _opt()
    learner = Learner(opt)
    keys, vals = learner.get_weights()
    ps = ddrl.ParameterServer(keys, vals)
    rb = ddrl.ReplayBufferNStep(opt)
    assert (rb.obs_dim, rb.act_dim) == (24, 4)
    opt.obs_dim, opt.act_dim = 8, 2            # the worker sets them from the model
    ro = ddrl.RolloutDeviceNStep(ps, rb, opt)
    assert (opt.obs_dim, opt.act_dim) == (24, 4)
    assert tuple(ro.act.shape) == (N, 4) and tuple(ro.env.obs.shape) == (N, 24) and ro.env.model == "walker" and ro.env.state_fields == 286
    assert (ro.winq.obs_dim, ro.winq.act_dim, ro.winq.Ln) == (24, 4, LN)
    assert [tuple(x.shape) for x in ro.winq.arrays] == [(N, LN + 1, 24), (N, LN, 4), (N, LN), (N, LN)]
    assert ro.limit_steps == LIMIT and ro._versions is False
    twin = _HandTwin(ddrl, ps, opt)
    steps, pushed = 25, 0
    policy_steps = 0
    for s in range(steps):
        policy_steps += int(ro.filling_steps > opt.start_steps)
        ro.step()
        twin.step()
        assert ro._fused is not True and ro._versions is False
        a, b = _snap(ro, rb), _snap(twin, twin.rb)
        assert a.keys() == b.keys()
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg="step %d: %s" % (s, k))
        assert ro.version == ps.version and ro.actor._noise_ctr == twin.actor._noise_ctr
        if s in (9, 16):                       # a push between two steps ...
            pushed += 1
            ps.push(keys, _perturbed(vals, pushed))
            assert ro.version != ps.version    # ... is not adopted before the next step, and by the whole vector after it (above)
    assert ro._fused is False                  # decided in the policy phase: no fused launch holds the walker
    assert ro.filling_steps == START + 1 and policy_steps == steps - (START + 1) and ro.actor._noise_ctr == policy_steps * N * 4
    from distributed_drl_amd.agent import Actor
    probe = torch.rand(N, 24, device="cuda")
    ref = Actor(opt, job="worker", max_rows=N)
    last = dict(zip(keys, _perturbed(vals, pushed)))
    ref.set_weights(ref.keys, [last[k] for k in ref.keys])
    assert torch.equal(ro.actor.get_actions(probe, deterministic=True), ref.get_actions(probe, deterministic=True))   # the last push's policy
    ptr, size, total = rb._counts()[:3]
    assert size == 150 and total >= size                                  # the ring is full (32 envs x 4 episodes x 3 windows: it wrapped)
    ep, _, ln = ro.env.stats()
    assert ep >= 3 * N and ln <= ep * LIMIT                               # every env ended episodes, none longer than the limit
    losses, _ = learner.train(rb.sample_batch(), return_outputs=True)
    v = np.array([float(x) for x in (losses.values() if isinstance(losses, dict) else losses)])
    assert len(v) >= 2 and np.isfinite(v).all(), losses
    assert learner._lib.ddrl_sac1_is_fused(learner._h) == 0               # obs + act = 28: the generic launch path


def test_the_ring_check_comes_before_any_allocation(ddrl):
    """A transition ring, and a window ring of another shape: ValueError naming the walker, and no env was created (the constructor
    left no env attribute behind, and the device holds no more memory than before)."""
    from distributed_drl_amd.workers import RolloutDeviceDQN, RolloutDeviceNStep
    opt = _opt()
    wrong = [ddrl.ReplayBufferSAC1(24, 4, 256, seed=0), ddrl.ReplayBufferNStep(_opt(8, 2))]
    good = ddrl.ReplayBufferNStep(_opt())
    made = []
    from distributed_drl_amd import env as env_mod
    real_init = env_mod.VecBipedalWalker.__init__

    def counting_init(self, *a, **kw):
        made.append(1)
        real_init(self, *a, **kw)

    env_mod.VecBipedalWalker.__init__ = counting_init
    try:
        for rbs in (wrong[0], [wrong[0]], wrong[1], [good, wrong[1]]):
            gc.collect()
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated()
            with pytest.raises(ValueError, match="walker"):
                RolloutDeviceNStep(None, rbs, opt)
            assert torch.cuda.memory_allocated() == before
        assert made == []
        with pytest.raises(ValueError, match="walker"):
            RolloutDeviceDQN(None, good, opt)       # the discrete worker keeps refusing the walker
        assert made == []
        ro = RolloutDeviceNStep(None, [good], opt)  # ... and the right ring is taken (ps=None: a rollout rank)
        assert made == [1] and ro.env.model == "walker" and ro._versions is False
        ro.step(2)
        assert ro.filling_steps == 2
    finally:
        env_mod.VecBipedalWalker.__init__ = real_init
