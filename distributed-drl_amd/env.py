"""Batched lander environment (device-resident) + the single-env facade the reference's loops use.

Stands where the reference calls `gym.make('LunarLanderContinuous-v2')`, `env.reset()`,
`env.step(a)` and `env.action_space.sample()` (example/dsac.py:78-79,99,102,127).  gym/Box2D are
not available; the dynamics are this build's own Box2D-style model (csrc/lander.hip; specification
and caveats in oracle/env_oracle.py's header and DESIGN.md §env).
"""
import ctypes

import numpy as np
import torch

from . import _lib


def _check_model(model):
    if model not in ("simple", "articulated"):
        raise ValueError("env model must be \"simple\" or \"articulated\": %r" % (model,))
    return model


class VecLunarLander:
    """n environments stepped by one kernel launch; all tensors stay on the device."""

    obs_dim, act_dim, act_high = 8, 2, 1.0

    def __init__(self, n_envs, seed=0, max_ep_len=1000, device=None, model="simple", velocity_iterations=180, position_iterations=60):
        """model: "simple" — the one-body lander (ddrl_env_create) — or "articulated" — hull and two jointed legs on Box2D's island
        solve with `velocity_iterations` / `position_iterations` sweeps (gym's world.Step arguments by default; ddrl_env_create_ex).
        The articulated env has reset / step / step_wrapped_articulated / stats / get_state / set_state; step_wrapped and the one-body
        fused rollout launches (ddrl_rollout_step, ddrl_rollout_step_discrete, ddrl_rollout_step_nstep) refuse it.  This model's own
        fused pairs are ddrl_rollout_begin_articulated / ddrl_rollout_step_articulated, reached through workers.RolloutDevice,
        ddrl_rollout_begin_discrete_articulated / ddrl_rollout_step_discrete_articulated, reached through workers.RolloutDeviceDQN
        (its mirrors: rollout_mirrors()), and ddrl_rollout_begin_nstep_articulated / ddrl_rollout_step_nstep_articulated, reached
        through workers.RolloutDeviceNStep.  Like the one-body model it is not pinned against gym (tests/lander3_oracle.py)."""
        _lib.require_gpu()
        self._lib = _lib.load()
        self.n, self.seed, self.max_ep_len = int(n_envs), int(seed) & 0xFFFFFFFF, int(max_ep_len)
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self.model = _check_model(model)
        h = ctypes.c_void_p()
        if self.model == "simple":
            _lib.check(self._lib.ddrl_env_create(ctypes.byref(h), self.device.index, self.n, self.seed, self.max_ep_len))
        else:
            m = _lib.EnvModel(_lib.DDRL_ENV_ARTICULATED, int(velocity_iterations), int(position_iterations))
            _lib.check(self._lib.ddrl_env_create_ex(ctypes.byref(h), self.device.index, self.n, self.seed, self.max_ep_len, ctypes.byref(m)))
        self._h = h
        self.state_fields = int(self._lib.ddrl_env_state_fields(h))
        e = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=self.device)
        self.obs = e(self.n, 8)        # observation to act on next
        self.obs2 = e(self.n, 8)       # o2 of the last transition
        self.rew, self.done = e(self.n), e(self.n)
        self.ended = e(self.n, dt=torch.uint8)
        self._sample_ctr = 0
        self.reset()

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.ddrl_env_destroy(h)

    def reset(self, mask=None):
        """env.reset() for every env (or those with mask != 0); returns obs[n, 8] (device)."""
        m = None if mask is None else mask.to(device=self.device, dtype=torch.uint8).contiguous()
        _lib.check(self._lib.ddrl_env_reset(self._h, _lib.dptr(m), _lib.dptr(self.obs), _lib.stream_ptr()))
        return self.obs

    def step(self, act):
        """env.step(a) for every env + episode bookkeeping of example/dsac.py:102-127.
        Returns (obs2, rew, done_as_stored, next_obs, ended) — device tensors owned by the env."""
        act = _lib.aligned(act.to(device=self.device, dtype=torch.float32).contiguous(), 8)   # ddrl.h: act_d is read as float2 rows
        _lib.check(self._lib.ddrl_env_step(self._h, _lib.dptr(act), _lib.dptr(self.obs2), _lib.dptr(self.rew),
                                           _lib.dptr(self.done), _lib.dptr(self.obs), _lib.dptr(self.ended),
                                           _lib.stream_ptr()))
        return self.obs2, self.rew, self.done, self.obs, self.ended

    def step_wrapped(self, act, act_noise=0.0, obs_noise=0.0, reward_scale=1.0, action_repeat=3, limit_steps=None):
        """env.step through `Wrapper` (algos/sac1/hyperparams.py:107-134) + the n-step rollout's episode
        bookkeeping (algos/sac1/sac_ray.py:212-258).  Same outputs as step(); done is the raw d.  `act` (a contiguous float32 device
        tensor) receives the noisy action in place, so a view that starts off the 8-byte grid is not copied: the library refuses it
        (ValueError naming act_d)."""
        act = act.to(device=self.device, dtype=torch.float32).contiguous()
        limit = int(limit_steps if limit_steps is not None else self.max_ep_len)
        _lib.check(self._lib.ddrl_env_step_wrapped(self._h, _lib.dptr(act), float(act_noise), float(obs_noise), float(reward_scale),
                                                   int(action_repeat), limit, _lib.dptr(self.obs2), _lib.dptr(self.rew),
                                                   _lib.dptr(self.done), _lib.dptr(self.obs), _lib.dptr(self.ended), _lib.stream_ptr()))
        return self.obs2, self.rew, self.done, self.obs, self.ended

    def step_wrapped_articulated(self, act, act_noise=0.0, obs_noise=0.0, reward_scale=1.0, action_repeat=3, limit_steps=None):
        """step_wrapped on the articulated lander (ddrl_env_step_wrapped_articulated, csrc/rollout3_nstep.hip): the same Wrapper and
        bookkeeping around the three-body solver with this env's iteration counts; same arguments and outputs, `act` updated in place.
        On model="simple" the library refuses (DdrlUnsupported naming step_wrapped's entry point); step_wrapped is unchanged and keeps
        refusing this model."""
        act = act.to(device=self.device, dtype=torch.float32).contiguous()
        limit = int(limit_steps if limit_steps is not None else self.max_ep_len)
        _lib.check(self._lib.ddrl_env_step_wrapped_articulated(self._h, _lib.dptr(act), float(act_noise), float(obs_noise),
                                                               float(reward_scale), int(action_repeat), limit, _lib.dptr(self.obs2),
                                                               _lib.dptr(self.rew), _lib.dptr(self.done), _lib.dptr(self.obs),
                                                               _lib.dptr(self.ended), _lib.stream_ptr()))
        return self.obs2, self.rew, self.done, self.obs, self.ended

    def sample_actions(self, out=None):
        """env.action_space.sample() for every env: U[-1, 1) from the counter generator."""
        out = out if out is not None else torch.empty(self.n, 2, dtype=torch.float32, device=self.device)
        _lib.check(self._lib.ddrl_uniform_fill(_lib.dptr(out), self.n * 2, -1.0, 1.0, self.seed ^ 0x5EED5EED,
                                               self._sample_ctr, _lib.stream_ptr()))
        self._sample_ctr += self.n * 2
        return out

    def stats(self):
        """(finished episodes, sum of returns, sum of lengths) since the last call."""
        ep, ln, rs = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_double()
        _lib.check(self._lib.ddrl_env_stats(self._h, ctypes.byref(ep), ctypes.byref(rs), ctypes.byref(ln),
                                            _lib.stream_ptr()))
        return int(ep.value), float(rs.value), int(ln.value)

    def get_state(self):
        s = torch.empty(self.state_fields, self.n, dtype=torch.float32, device=self.device)
        _lib.check(self._lib.ddrl_env_get_state(self._h, _lib.dptr(s), _lib.stream_ptr()))
        return s

    def set_state(self, s):
        s = s.to(device=self.device, dtype=torch.float32).contiguous()
        if tuple(s.shape) != (self.state_fields, self.n):
            raise ValueError("state block must be [%d, %d] for this env's model, got %s" % (self.state_fields, self.n, tuple(s.shape)))
        _lib.check(self._lib.ddrl_env_set_state(self._h, _lib.dptr(s), _lib.stream_ptr()))

    def rollout_mirrors(self):
        """(act [n], q [n, A], next_obs [n, 8]): device views of the block the env handle owns for the articulated lander's fused
        discrete rollout step (ddrl_env_rollout_mirrors) — the last step's action indices, its Q rows and the observations to act on
        next.  No copy and no synchronisation: the views are stream-ordered like any tensor, and valid for the handle's life (the
        block is never moved).  Before any ddrl_rollout_begin_discrete_articulated on this env the library refuses (ValueError)."""
        act, q, nxt = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        n, A = ctypes.c_int32(), ctypes.c_int32()
        _lib.check(self._lib.ddrl_env_rollout_mirrors(self._h, ctypes.byref(act), ctypes.byref(q), ctypes.byref(nxt), ctypes.byref(n),
                                                      ctypes.byref(A)))
        n, A = int(n.value), int(A.value)
        return (_device_view(act.value, n, "<f4", self.device), _device_view(q.value, n * A, "<f4", self.device).view(n, A),
                _device_view(nxt.value, n * 8, "<f4", self.device).view(n, 8))


class VecBipedalWalker(VecLunarLander):
    """n bipedal walkers stepped by one kernel launch (ddrl_env_create_ex, kind DDRL_ENV_WALKER; csrc/walker.hip): gym's BipedalWalker
    shape — hull, two two-segment legs on four motorised joints, 10 lidar rays, 24 observations, 4 actions — on the articulated
    lander's solver with `velocity_iterations` / `position_iterations` sweeps (gym's world.Step arguments by default).  Specification,
    and what is gym's, Box2D's and this build's own: tests/walker_oracle.py.  NOT pinned against gym.  It has reset / step /
    step_wrapped_walker (the n-step worker's step, csrc/walker.hip) / sample_actions / stats / get_state / set_state; the
    landers' wrapped steps (the inherited step_wrapped and step_wrapped_articulated), every fused rollout launch and the landers'
    on-device evaluation (ddrl_env_eval_policy / ddrl_env_eval_q) hold a lander, and the library refuses this env there (DdrlUnsupported
    naming the entry point and the walker).  Its evaluation episodes run on the device through a door of their own: the marker
    DeviceBipedalWalker and Actor.evaluate_env (ddrl_env_eval_policy_walker, csrc/walker_eval.hip), which borrows a handle of this class.
    terrain="hardcore" (ddrl_env_create_walker, include/ddrl_walker_hardcore.h; csrc/walker.hip; specification
    tests/walker_hardcore_oracle.py): gym's BipedalWalkerHardcore terrain generator — stumps, pits and stairs as boxes, a second (wall)
    contact slot per leg corner, a hull that ends the episode inside a box, lidar rays that see box edges — behind every method above,
    with a state block of `state_fields` = 663 rows.  Its evaluation episodes run on the device through the marker
    DeviceBipedalWalkerHardcore (ddrl_env_eval_policy_walker_hardcore, csrc/walker_hardcore_eval.hip); the grass terrain's entry point
    refuses such a handle (DdrlUnsupported naming the hardcore terrain), as the Hardcore one refuses a grass handle.
    terrain="grass" is the env it always was, bit for bit."""

    obs_dim, act_dim, act_high = 24, 4, 1.0
    model = "walker"
    TERRAINS = {"grass": _lib.DDRL_WALKER_TERRAIN_GRASS, "hardcore": _lib.DDRL_WALKER_TERRAIN_HARDCORE}

    def __init__(self, n_envs, seed=0, max_ep_len=1600, device=None, velocity_iterations=180, position_iterations=60, model="walker",
                 terrain="grass"):
        if model != "walker":   # (taken so that every class of MODELS is built with the same keywords)
            raise ValueError("VecBipedalWalker is the env of model=\"walker\": %r" % (model,))
        if terrain not in self.TERRAINS:
            raise ValueError("VecBipedalWalker: terrain must be \"grass\" or \"hardcore\", got %r" % (terrain,))
        self.terrain = terrain
        _lib.require_gpu()
        self._lib = _lib.load()
        self.n, self.seed, self.max_ep_len = int(n_envs), int(seed) & 0xFFFFFFFF, int(max_ep_len)
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        h = ctypes.c_void_p()
        if terrain == "grass":
            m = _lib.EnvModel(_lib.DDRL_ENV_WALKER, int(velocity_iterations), int(position_iterations))
            _lib.check(self._lib.ddrl_env_create_ex(ctypes.byref(h), self.device.index, self.n, self.seed, self.max_ep_len, ctypes.byref(m)))
        else:
            _lib.check(self._lib.ddrl_env_create_walker(ctypes.byref(h), self.device.index, self.n, self.seed, self.max_ep_len,
                                                        int(velocity_iterations), int(position_iterations), self.TERRAINS[terrain]))
        self._h = h
        self.state_fields = int(self._lib.ddrl_env_state_fields(h))
        e = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=self.device)
        self.obs = e(self.n, self.obs_dim)        # observation to act on next
        self.obs2 = e(self.n, self.obs_dim)       # o2 of the last transition
        self.rew, self.done = e(self.n), e(self.n)
        self.ended = e(self.n, dt=torch.uint8)
        self._sample_ctr = 0
        self.reset()

    def step(self, act):
        """env.step(a) for every env (a: [n, 4], gym's hip / knee / hip / knee motor commands) + the bookkeeping of VecLunarLander.step;
        same outputs, observations [n, 24]."""
        act = act.to(device=self.device, dtype=torch.float32).contiguous()
        if tuple(act.shape) != (self.n, self.act_dim):
            raise ValueError("the walker's actions are [%d, %d], got %s" % (self.n, self.act_dim, tuple(act.shape)))
        act = _lib.aligned(act, 16)   # ddrl.h: a walker's act_d is read as float4 rows
        _lib.check(self._lib.ddrl_env_step(self._h, _lib.dptr(act), _lib.dptr(self.obs2), _lib.dptr(self.rew),
                                           _lib.dptr(self.done), _lib.dptr(self.obs), _lib.dptr(self.ended),
                                           _lib.stream_ptr()))
        return self.obs2, self.rew, self.done, self.obs, self.ended

    def step_wrapped_walker(self, act, act_noise=0.0, obs_noise=0.0, reward_scale=1.0, action_repeat=3, limit_steps=None):
        """step_wrapped on the walker (ddrl_env_step_wrapped_walker, csrc/walker.hip; specification
        tests/walker_wrapped_oracle.py): the same Wrapper and bookkeeping around the five-body solver with this env's iteration counts;
        same arguments and outputs as step_wrapped_articulated, observations [n, 24], done the raw d.  `act` ([n, 4], a contiguous
        float32 device tensor) receives the noisy action in place.  The library reads and writes an action row as one float4, so `act`
        goes through _lib.aligned(act, 16) as in step(): a view that starts off the 16-byte grid is staged in an aligned copy, and the
        noisy action is copied back into the view on the same stream — the caller sees the in-place update either way, at the cost of
        two copies for such a view.  (A tensor on another device or of another dtype is converted first and is NOT written back, as in
        step_wrapped.)  The inherited step_wrapped and step_wrapped_articulated keep raising DdrlUnsupported on this env."""
        given = act
        act = act.to(device=self.device, dtype=torch.float32).contiguous()
        if tuple(act.shape) != (self.n, self.act_dim):
            raise ValueError("the walker's actions are [%d, %d], got %s" % (self.n, self.act_dim, tuple(act.shape)))
        a = _lib.aligned(act, 16)
        limit = int(limit_steps if limit_steps is not None else self.max_ep_len)
        _lib.check(self._lib.ddrl_env_step_wrapped_walker(self._h, _lib.dptr(a), float(act_noise), float(obs_noise), float(reward_scale),
                                                          int(action_repeat), limit, _lib.dptr(self.obs2), _lib.dptr(self.rew),
                                                          _lib.dptr(self.done), _lib.dptr(self.obs), _lib.dptr(self.ended),
                                                          _lib.stream_ptr()))
        if act is given and a is not act:
            act.copy_(a)
        return self.obs2, self.rew, self.done, self.obs, self.ended

    def sample_actions(self, out=None):
        """env.action_space.sample() for every env: U[-1, 1) from the counter generator."""
        out = out if out is not None else torch.empty(self.n, self.act_dim, dtype=torch.float32, device=self.device)
        _lib.check(self._lib.ddrl_uniform_fill(_lib.dptr(out), self.n * self.act_dim, -1.0, 1.0, self.seed ^ 0x5EED5EED,
                                               self._sample_ctr, _lib.stream_ptr()))
        self._sample_ctr += self.n * self.act_dim
        return out


class VecLunarLanderDiscrete(VecLunarLander):
    """The same n landers behind gym's discrete LunarLander-v2 action table (ddrl_env_step_discrete): 0 noop, 1 left engine,
    2 main engine, 3 right engine — under the continuous step's clip rules exactly gym's discrete powers, so no new dynamics.  The env
    is this project's own one-body lander (see the module header), the table is gym's.  Actions are indices as float32 [n], the
    form the DQN replay ring stores."""

    act_dim = 4

    def step(self, idx):
        """env.step(a) for every env on the action table; outputs and bookkeeping of VecLunarLander.step."""
        idx = idx.to(device=self.device, dtype=torch.float32).contiguous()
        assert idx.numel() == self.n
        _lib.check(self._lib.ddrl_env_step_discrete(self._h, _lib.dptr(idx), _lib.dptr(self.obs2), _lib.dptr(self.rew),
                                                    _lib.dptr(self.done), _lib.dptr(self.obs), _lib.dptr(self.ended), _lib.stream_ptr()))
        return self.obs2, self.rew, self.done, self.obs, self.ended

    def step_wrapped(self, *a, **kw):
        raise NotImplementedError("the SAC1 wrapper acts on continuous actions: VecLunarLander.step_wrapped")

    def sample_actions(self, out=None):
        """env.action_space.sample() for every env: floor of U[0, 4) from the counter generator."""
        out = out if out is not None else torch.empty(self.n, dtype=torch.float32, device=self.device)
        _lib.check(self._lib.ddrl_uniform_fill(_lib.dptr(out), self.n, 0.0, 4.0, self.seed ^ 0x5EED5EED, self._sample_ctr, _lib.stream_ptr()))
        self._sample_ctr += self.n
        return torch.floor_(out)


# The C entry points of each env model, by `env.model`: what workers.py reads where a worker's calls depend on the model (the library's
# side of this table is csrc/env.hip's model table).  cls: the vectorised env of the continuous workers; dims: the (obs_dim, act_dim) its
# worker writes into its options (None: the options keep theirs — a lander's policy may have one action or two); wrapped: the env's wrapped-step method; fused: per fused family — "pi" (RolloutDevice), "q" (RolloutDeviceDQN), "nstep"
# (RolloutDeviceNStep) — the (begin, step) entry-point NAMES, whether the pair is opt-in (taken only where the worker's own
# `opt.fused_*_articulated` flag is set) and whether the step takes handles only, its mirrors being a block the env handle owns (rollout_mirrors).  A
# family is missing where no fused launch holds the model.  eval: the handle-fed evaluation of a continuous policy (Actor.evaluate_env) —
# the entry point's NAME and the floats of its trace row, as eval_results reads them.
MODELS = {
    "simple": dict(cls=VecLunarLander, dims=None, wrapped="step_wrapped", eval=("ddrl_env_eval_policy", 12), fused={
        "pi": ("ddrl_rollout_begin", "ddrl_rollout_step", False, False),
        "q": ("ddrl_rollout_begin_discrete", "ddrl_rollout_step_discrete", False, False),
        "nstep": ("ddrl_rollout_begin_nstep", "ddrl_rollout_step_nstep", False, False)}),
    "articulated": dict(cls=VecLunarLander, dims=None, wrapped="step_wrapped_articulated", eval=("ddrl_env_eval_policy", 12), fused={
        "pi": ("ddrl_rollout_begin_articulated", "ddrl_rollout_step_articulated", True, False),
        "q": ("ddrl_rollout_begin_discrete_articulated", "ddrl_rollout_step_discrete_articulated", True, True),
        "nstep": ("ddrl_rollout_begin_nstep_articulated", "ddrl_rollout_step_nstep_articulated", True, False)}),
    "walker": dict(cls=VecBipedalWalker, dims=(24, 4), wrapped="step_wrapped_walker", eval=("ddrl_env_eval_policy_walker", 32), fused={}),
}


class _ActionSpace:
    def __init__(self, env):
        self._env = env
        self.high = np.array([1.0, 1.0], dtype=np.float32)
        self.low = -self.high
        self.shape = (2,)

    def sample(self):
        return self._env._vec.sample_actions()[0].cpu().numpy()


class _ObsSpace:
    shape = (8,)


class LunarLander:
    """One environment with the gym call shape (reset() -> o; step(a) -> (o2, r, d, info)) for the
    reference-style loops (worker_rollout with num_envs == 1, worker_test).  `d` is True at the
    time limit too, as gym's TimeLimit wrapper reports it."""

    def __init__(self, seed=0, max_ep_len=1000, model="simple", velocity_iterations=180, position_iterations=60):
        self._vec = VecLunarLander(1, seed=seed, max_ep_len=max_ep_len, model=model, velocity_iterations=velocity_iterations,
                                   position_iterations=position_iterations)
        self.action_space = _ActionSpace(self)
        self.observation_space = _ObsSpace()
        self._fresh = True  # the kernel resets finished envs itself

    def reset(self):
        if not self._fresh:
            self._vec.reset()
        self._fresh = False
        return self._vec.obs[0].cpu().numpy().astype(np.float64)

    def step(self, a):
        act = torch.as_tensor(np.asarray(a, np.float32).reshape(1, 2))
        o2, r, d, _, ended = self._vec.step(act)
        ended = bool(ended[0].item())
        self._fresh = ended
        return o2[0].cpu().numpy().astype(np.float64), float(r[0].item()), ended, {}


class _WalkerActionSpace(_ActionSpace):
    def __init__(self, env):
        self._env = env
        self.high = np.ones(4, dtype=np.float32)
        self.low = -self.high
        self.shape = (4,)


class _WalkerObsSpace:
    shape = (24,)


class BipedalWalker(LunarLander):
    """One walker with the gym call shape (env.make("BipedalWalker-v2", model="walker")): reset() -> o[24]; step(a[4]) -> (o2, r, d,
    info), `d` True at the time limit too (gym's TimeLimit of 1600 is max_ep_len).  terrain="hardcore"
    (env.make("BipedalWalkerHardcore-v2", model="walker", terrain="hardcore")): VecBipedalWalker's Hardcore terrain."""

    def __init__(self, seed=0, max_ep_len=1600, velocity_iterations=180, position_iterations=60, terrain="grass"):
        self._vec = VecBipedalWalker(1, seed=seed, max_ep_len=max_ep_len, velocity_iterations=velocity_iterations,
                                     position_iterations=position_iterations, terrain=terrain)
        self.action_space = _WalkerActionSpace(self)
        self.observation_space = _WalkerObsSpace()
        self._fresh = True

    def step(self, a):
        act = torch.as_tensor(np.asarray(a, np.float32).reshape(1, 4))
        o2, r, d, _, ended = self._vec.step(act)
        ended = bool(ended[0].item())
        self._fresh = ended
        return o2[0].cpu().numpy().astype(np.float64), float(r[0].item()), ended, {}


class _DiscreteActionSpace:
    n, shape = 4, ()

    def __init__(self, env):
        self._env = env

    def sample(self):
        return int(self._env._vec.sample_actions()[0].item())


class LunarLanderDiscrete(LunarLander):
    """One discrete-action environment with the gym call shape (env.make("LunarLander-v2")): step(a) takes the action index.
    `rewards[0]` is the Python-float sum of the step rewards since the last reset() (0.0 after one): the score dqn.Actor.test reads
    at every episode's end (algos/dqn/actor_learner.py:246; the trading env's bookkeeping) — on the lander, the episode's return."""

    def __init__(self, seed=0, max_ep_len=1000, model="simple", velocity_iterations=180, position_iterations=60):
        self._vec = VecLunarLanderDiscrete(1, seed=seed, max_ep_len=max_ep_len, model=model, velocity_iterations=velocity_iterations,
                                           position_iterations=position_iterations)
        self.action_space = _DiscreteActionSpace(self)
        self.observation_space = _ObsSpace()
        self._fresh = True
        self.rewards = [0.0]

    def reset(self):
        self.rewards = [0.0]
        return super().reset()

    def step(self, a):
        o2, r, d, _, ended = self._vec.step(torch.full((1,), float(int(a)), dtype=torch.float32))
        ended = bool(ended[0].item())
        self._fresh = ended
        r = float(r[0].item())
        self.rewards[0] += r
        return o2[0].cpu().numpy().astype(np.float64), r, ended, {}


class DeviceLunarLander:
    """The test env of an on-device evaluation: a MARKER, not a steppable env.  It holds what names the episodes a host
    `LunarLander(seed, max_ep_len, model=...)` would play one after another — the seed, the model and how many episodes have been
    played — and `Actor.test` / `Model.test_agent` given one run their episodes as one launch and advance the count: on the one-body
    lander (model="simple") `Actor.evaluate` (ddrl_policy_eval, csrc/eval.hip), on the articulated lander `Actor.evaluate_env`
    (ddrl_env_eval_policy, csrc/eval3.hip), which borrows `handle()`: a one-env handle of the marker's model, created at the first
    use, that names the model to the library and owns the results block.  Its env state is never stepped.
    reset / action_space exist so that nothing breaks on attribute access at construction; step raises."""

    on_device = True

    def __init__(self, seed=0, max_ep_len=1000, *, model="simple", velocity_iterations=180, position_iterations=60):
        self.seed, self.max_ep_len = int(seed) & 0xFFFFFFFF, int(max_ep_len)
        self.model = _check_model(model)
        self.velocity_iterations, self.position_iterations = int(velocity_iterations), int(position_iterations)
        self.episodes_played = 0
        self.action_space = _ActionSpace(self)
        self.observation_space = _ObsSpace()
        self._lend = None

    def _model_kw(self):
        if self.model == "simple":
            return {}
        return dict(model=self.model, velocity_iterations=self.velocity_iterations, position_iterations=self.position_iterations)

    def reset(self):
        return np.zeros(8, np.float64)

    def step(self, a):
        raise RuntimeError("DeviceLunarLander is not steppable: its episodes run on the device (Actor.evaluate / Actor.test / "
                           "Model.test_agent); use env.make(name) for an env to step from the host")

    def handle(self):
        """The one-env handle (a VecLunarLander of this marker's seed, max_ep_len and model) lent to ddrl_env_eval_policy /
        ddrl_env_eval_q; created on first use."""
        if self._lend is None:
            self._lend = VecLunarLander(1, seed=self.seed, max_ep_len=self.max_ep_len, **self._model_kw())
        return self._lend

    def host_env(self):
        """A host env of the same seed and model positioned at the next episode this env would play (the fallback of a policy
        outside the evaluation kernels' envelope)."""
        host = self._host_class(self.seed, self.max_ep_len, **self._model_kw())
        if self.episodes_played:
            s = host._vec.get_state()
            # EPI: the episode index names the env's random stream.  Field 13 in BOTH layouts (csrc/env_device.h's enum, which
            # env3_device.h's load / store index with too; tests/lander3_oracle.py keeps it there for this line)
            s[13] = float(self.episodes_played)
            host._vec.set_state(s)
            host._vec.reset()
        return host

    _host_class = LunarLander


class DeviceLunarLanderDiscrete(DeviceLunarLander):
    """The same marker for the discrete lander (action_space.n == 4): `dqn.Actor.test` / `ActorSQN.test` given one run their episodes
    as one launch (`evaluate`, csrc/eval_q.hip; on the articulated model `evaluate_env`, csrc/eval3.hip); host_env() is a
    `LunarLanderDiscrete` positioned at `episodes_played`."""

    _host_class = LunarLanderDiscrete

    def __init__(self, seed=0, max_ep_len=1000, **model_kw):
        super().__init__(seed, max_ep_len, **model_kw)
        self.action_space = _DiscreteActionSpace(self)

    def step(self, a):
        raise RuntimeError("DeviceLunarLanderDiscrete is not steppable: its episodes run on the device (dqn.Actor.evaluate / "
                           "dqn.Actor.test); use env.make(\"LunarLander-v2\") for an env to step from the host")


class DeviceBipedalWalker(DeviceLunarLander):
    """The same marker for the WALKER (model "walker"; 24 observations, 4 actions): `Actor.test` given one runs its episodes as one
    launch — `Actor.evaluate_env` (ddrl_env_eval_policy_walker, csrc/walker_eval.hip), one workgroup per episode — and advances
    `episodes_played`.  Episode e is the e-th a host `BipedalWalker(seed, max_ep_len, velocity_iterations, position_iterations)` plays.
    handle() is a one-env VecBipedalWalker, created on first use, that names the model to the library and owns the results block;
    host_env() is a `BipedalWalker` positioned at `episodes_played` (EPI is field 13 in this layout too: csrc/walker_device.h loads
    and stores it by csrc/env_device.h's enum).  Built by name, not by env.make / env.make_device, which keep refusing the walker;
    workers._default_test_env builds it for `opt.env_model = "walker"` under `opt.test_on_device`.  terrain="hardcore" raises
    ValueError: this marker's evaluation kernel holds the grass terrain; the Hardcore terrain's marker is DeviceBipedalWalkerHardcore."""

    _host_class = BipedalWalker
    terrain = "grass"

    def __init__(self, seed=0, max_ep_len=1600, velocity_iterations=180, position_iterations=60, terrain="grass"):
        if terrain != "grass":
            raise ValueError("DeviceBipedalWalker(terrain=%r): this marker holds the grass terrain — its evaluation kernel "
                             "(ddrl_env_eval_policy_walker, csrc/walker_eval.hip) builds that one; the Hardcore terrain's is "
                             "ddrl_env_eval_policy_walker_hardcore (csrc/walker_hardcore_eval.hip), reached through "
                             "env.DeviceBipedalWalkerHardcore(seed, max_ep_len, velocity_iterations, position_iterations)" % (terrain,))
        self.seed, self.max_ep_len, self.model = int(seed) & 0xFFFFFFFF, int(max_ep_len), "walker"
        self.velocity_iterations, self.position_iterations = int(velocity_iterations), int(position_iterations)
        self.episodes_played = 0
        self.action_space = _WalkerActionSpace(self)
        self.observation_space = _WalkerObsSpace()
        self._lend = None

    def _model_kw(self):   # BipedalWalker and VecBipedalWalker are the model: they take the iteration counts only
        return dict(velocity_iterations=self.velocity_iterations, position_iterations=self.position_iterations)

    def reset(self):
        return np.zeros(24, np.float64)

    def step(self, a):
        raise RuntimeError("DeviceBipedalWalker is not steppable: its episodes run on the device (Actor.evaluate_env / Actor.test); "
                           "use env.make(\"BipedalWalker-v2\", model=\"walker\") for an env to step from the host")

    def handle(self):
        """The one-env handle (a VecBipedalWalker of this marker's seed, max_ep_len and iteration counts) lent to
        ddrl_env_eval_policy_walker; created on first use."""
        if self._lend is None:
            self._lend = VecBipedalWalker(1, seed=self.seed, max_ep_len=self.max_ep_len, **self._model_kw())
        return self._lend


class DeviceBipedalWalkerHardcore(DeviceBipedalWalker):
    """DeviceBipedalWalker's twin for the HARDCORE terrain (model "walker", terrain "hardcore": stumps, pits, stairs): `Actor.test` given
    one runs its episodes as one launch — `Actor.evaluate_env` through `eval_entry` (ddrl_env_eval_policy_walker_hardcore,
    csrc/walker_hardcore_eval.hip), one workgroup per episode, the episode's terrain generated inside the kernel — and advances
    `episodes_played`.  Episode e is the e-th a host `BipedalWalker(seed, max_ep_len, velocity_iterations, position_iterations,
    terrain="hardcore")` plays (env.make("BipedalWalkerHardcore-v2", model="walker", terrain="hardcore")).  handle() is a one-env
    VecBipedalWalker(terrain="hardcore"), host_env() a BipedalWalker(terrain="hardcore") positioned at `episodes_played`.
    The marker names its entry point itself (`eval_entry`: the name and the floats of a trace row), which Actor.evaluate_env prefers
    to env.MODELS[model]["eval"]: the terrain is no model, and the table keeps the grass walker's entry point.  Built by name, like the
    grass marker; workers._default_test_env builds it for `opt.env_model = "walker"`, `opt.env_terrain = "hardcore"` under
    `opt.test_on_device_hardcore`."""

    terrain = "hardcore"
    eval_entry = ("ddrl_env_eval_policy_walker_hardcore", 32)

    def __init__(self, seed=0, max_ep_len=1600, velocity_iterations=180, position_iterations=60):
        super().__init__(seed, max_ep_len, velocity_iterations, position_iterations)

    def _model_kw(self):
        return dict(super()._model_kw(), terrain="hardcore")

    def step(self, a):
        raise RuntimeError("DeviceBipedalWalkerHardcore is not steppable: its episodes run on the device (Actor.evaluate_env / Actor.test); "
                           "use env.make(\"BipedalWalkerHardcore-v2\", model=\"walker\", terrain=\"hardcore\") for an env to step from "
                           "the host")


def _device_view(ptr, count, typestr, device):
    """`count` elements of device memory the library owns as a flat tensor (a __cuda_array_interface__ view: no copy, no ownership)."""
    class _Holder:
        __cuda_array_interface__ = {"shape": (count,), "typestr": typestr, "data": (int(ptr), False), "version": 2}
    return torch.as_tensor(_Holder(), device=device)


def eval_results(vec, want_row):
    """The results of the last ddrl_env_eval_policy / ddrl_env_eval_q / ddrl_env_eval_policy_walker / _walker_hardcore on `vec` (a VecLunarLander or a
    VecBipedalWalker; want_row: 12, 20 or 32) as NumPy: dict(ret float64 [n],
    len int32 [n]) and, where that call kept a trace, `trace` float32 [n, max_ep_len, want_row].  Read from the block the env handle
    owns (ddrl_env_eval_results) through __cuda_array_interface__ views, as replay.py reads its rings; synchronises the stream."""
    ret, ln, tr = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    n, L, row = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    _lib.check(vec._lib.ddrl_env_eval_results(vec._h, ctypes.byref(ret), ctypes.byref(ln), ctypes.byref(tr), ctypes.byref(n),
                                              ctypes.byref(L), ctypes.byref(row)))
    n, L, row = int(n.value), int(L.value), int(row.value)
    view = lambda ptr, count, typestr: _device_view(ptr, count, typestr, vec.device)
    torch.cuda.current_stream().synchronize()
    out = {"ret": view(ret.value, n, "<f8").cpu().numpy(), "len": view(ln.value, n, "<i4").cpu().numpy()}
    if row:
        if row != want_row:
            raise _lib.DdrlError("the env handle's last evaluation kept a trace of %d floats per step, not %d" % (row, want_row))
        out["trace"] = view(tr.value, n * L * row, "<f4").cpu().numpy().reshape(n, L, row)
    return out


class Wrapper(object):
    """algos/sac1/hyperparams.py:107-134 on a host env: uniform action noise added IN PLACE to the caller's action (`action +=`),
    the action repeated `action_repeat` times with the rewards summed and scaled — except that a terminal inside the repeat returns
    reward 0.0, and action_repeat == 1 returns the first step's raw reward and un-noised observation (the reference's branches, kept
    as they are).  The reference hard-codes BipedalWalker's sizes (24 observations, 4 actions) for the noise; here they follow the
    arrays.  `rng`: np.random (the reference) or a seeded RandomState."""

    def __init__(self, env, obs_noise, act_noise, reward_scale, action_repeat=3, rng=None):
        self._env = env
        self.action_repeat = action_repeat
        self.act_noise = act_noise
        self.obs_noise = obs_noise
        self.reward_scale = reward_scale
        self._rng = np.random if rng is None else rng

    def __getattr__(self, name):
        return getattr(self._env, name)

    def _noisy(self, obs):
        obs = np.asarray(obs)
        return obs + self.obs_noise * (-2 * self._rng.random_sample(obs.shape[-1]) + 1)

    def reset(self):
        return self._noisy(self._env.reset())

    def step(self, action):
        action += self.act_noise * (-2 * self._rng.random_sample(np.asarray(action).shape[-1]) + 1)
        r = 0.0
        for _ in range(self.action_repeat):
            obs_, reward_, done_, info_ = self._env.step(action)
            r = r + reward_
            if done_ and self.action_repeat != 1:
                return self._noisy(obs_), 0.0, done_, info_
            if self.action_repeat == 1:
                return obs_, r, done_, info_
        return self._noisy(obs_), self.reward_scale * r, done_, info_


def _walker_door(env_name, kw, who):
    """None for a lander name; for "BipedalWalker-v2" the BipedalWalker's keyword arguments.  The walker is asked for by name AND by
    model="walker": the bare name keeps raising ValueError, as it did before this env existed, because what stands behind it is this
    build's own model, unpinned against gym's (tests/walker_oracle.py) — a driver that names gym's env says so once, in its make call.
    "BipedalWalkerHardcore-v2" (pits, stumps, stairs: tests/walker_hardcore_oracle.py, unpinned likewise) needs one more word,
    terrain="hardcore": name and terrain have to agree, so neither the Hardcore name alone nor "BipedalWalker-v2" with
    terrain="hardcore" opens it."""
    if "BipedalWalker" not in env_name:
        if kw.get("model") == "walker":
            raise ValueError("%s(%r, model=\"walker\"): the walker's name is \"BipedalWalker-v2\"" % (who, env_name))
        return None
    terrain = kw.get("terrain", "grass")
    if env_name == "BipedalWalkerHardcore-v2":
        if terrain != "hardcore" or kw.get("model") != "walker":
            raise ValueError("%s(%r) needs model=\"walker\" and terrain=\"hardcore\": the Hardcore terrain (pits, stumps, stairs) is this "
                             "build's own model of it, not pinned against gym's" % (who, env_name))
        return {k: v for k, v in kw.items() if k != "model"}
    if env_name != "BipedalWalker-v2":
        raise ValueError("%s(%r): the walkers that are built are \"BipedalWalker-v2\" and \"BipedalWalkerHardcore-v2\"" % (who, env_name))
    if terrain != "grass":
        raise ValueError("%s(\"BipedalWalker-v2\", terrain=%r): name and terrain do not agree — \"BipedalWalker-v2\" is the grass "
                         "terrain; the Hardcore terrain's name is \"BipedalWalkerHardcore-v2\"" % (who, terrain))
    if kw.get("model") != "walker":
        raise ValueError("%s(\"BipedalWalker-v2\") needs model=\"walker\": the env behind the name is this build's own five-body model, "
                         "not pinned against gym's (only the LunarLanderContinuous-v2 stand-in is built without one; SURVEY §8(a) A7)" % who)
    return {k: v for k, v in kw.items() if k != "model"}


def _walker_marker_of(walker_kw):
    """(the evaluation entry point and its file, the marker's class name) of the terrain a walker door was asked for: what the two
    doors below name when they refuse to build a marker."""
    if walker_kw.get("terrain", "grass") == "hardcore":
        return "ddrl_env_eval_policy_walker_hardcore, csrc/walker_hardcore_eval.hip", "DeviceBipedalWalkerHardcore"
    return "ddrl_env_eval_policy_walker, csrc/walker_eval.hip", "DeviceBipedalWalker"


def make(env_name="LunarLanderContinuous-v2", on_device=False, **kw):
    """gym.make stand-in (example/dsac.py:78).  model="simple" | "articulated" (+ velocity_iterations, position_iterations) is passed on to the env.  "LunarLander-v2": the discrete single-env facade.  on_device=True: the test-env marker whose episodes `Actor.test` /
    `Model.test_agent` run as one launch (DeviceLunarLander; "LunarLander-v2": DeviceLunarLanderDiscrete for dqn.Actor.test / ActorSQN.test)
    on the one-body lander; the articulated model's marker is built by make_device.
    "BipedalWalker-v2" with model="walker" (+ seed, max_ep_len, velocity_iterations, position_iterations): the BipedalWalker facade
    (_walker_door); on_device=True raises: the walker's evaluation kernel is reached through env.DeviceBipedalWalker, not this door.
    "BipedalWalkerHardcore-v2" with model="walker" AND terrain="hardcore": the same facade on the Hardcore terrain (on_device=True
    raises likewise: that terrain's marker is env.DeviceBipedalWalkerHardcore)."""
    walker = _walker_door(env_name, kw, "env.make")
    if walker is not None:
        if on_device:
            raise ValueError("env.make(%r, on_device=True): this door builds the landers' markers only (ddrl_env_eval_policy / ddrl_env_eval_q, "
                             "csrc/eval3.hip, run landers) — the evaluation kernel for the walker (%s) is reached through env.%s(seed, "
                             "max_ep_len, velocity_iterations, position_iterations) and Actor.test / Actor.evaluate_env; use "
                             "on_device=False for a host-stepped env.make(%r, model=\"walker\")"
                             % ((env_name,) + _walker_marker_of(walker) + (env_name,)))
        return BipedalWalker(**walker)
    if on_device and _check_model(kw.get("model", "simple")) != "simple":
        raise ValueError("env.make(on_device=True, model=%r): this door builds the one-body lander's marker only (ddrl_policy_eval, csrc/eval.hip; "
                         "ddrl_dqn_eval, csrc/eval_q.hip) — the evaluation kernel for the articulated model (ddrl_env_eval_policy / "
                         "ddrl_env_eval_q, csrc/eval3.hip) is reached through env.make_device(env_name, model=%r, ...); "
                         "use on_device=False for a host-stepped env of that model" % (kw.get("model"), kw.get("model")))
    if on_device:
        kw = {k: v for k, v in kw.items() if k not in ("model", "velocity_iterations", "position_iterations")}
    if env_name == "LunarLander-v2":   # gym's discrete action table on the same lander (action_space.n == 4)
        return DeviceLunarLanderDiscrete(**kw) if on_device else LunarLanderDiscrete(**kw)
    if "LunarLander" not in env_name:
        raise ValueError("only the LunarLanderContinuous-v2 stand-in is built (SURVEY §8(a) A7): %r" % env_name)
    return DeviceLunarLander(**kw) if on_device else LunarLander(**kw)


def make_device(env_name="LunarLanderContinuous-v2", **kw):
    """The test-env marker of an on-device evaluation for EITHER model: seed, max_ep_len and model="simple" | "articulated"
    (+ velocity_iterations, position_iterations) as env.make takes them.  "LunarLander-v2": DeviceLunarLanderDiscrete (dqn.Actor.test /
    ActorSQN.test), else DeviceLunarLander (Actor.test / Model.test_agent).  The one-body marker is what make(on_device=True) returns.
    "BipedalWalker-v2" raises: the walker's marker is env.DeviceBipedalWalker ("BipedalWalkerHardcore-v2": env.DeviceBipedalWalkerHardcore)."""
    walker = _walker_door(env_name, kw, "env.make_device")
    if walker is not None:
        raise ValueError("env.make_device(%r): this door builds the landers' markers only (ddrl_env_eval_policy / ddrl_env_eval_q, "
                         "csrc/eval3.hip, run landers) — the evaluation kernel for the walker (%s) is reached through env.%s(seed, "
                         "max_ep_len, velocity_iterations, position_iterations) and Actor.test / Actor.evaluate_env; a host-stepped env "
                         "is env.make(%r, model=\"walker\")" % ((env_name,) + _walker_marker_of(walker) + (env_name,)))
    _check_model(kw.get("model", "simple"))
    if env_name == "LunarLander-v2":
        return DeviceLunarLanderDiscrete(**kw)
    if "LunarLander" not in env_name:
        raise ValueError("only the LunarLanderContinuous-v2 stand-in is built (SURVEY §8(a) A7): %r" % env_name)
    return DeviceLunarLander(**kw)
