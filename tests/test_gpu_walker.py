"""GPU parity of the BIPEDAL WALKER (ddrl_env_create_ex, kind = DDRL_ENV_WALKER; csrc/walker_device.h) vs its specification
tests/walker_oracle.py — BIT-EXACT, live at 8 / 3 iterations and against the golden file at gym's 180 / 60 — plus the C-ABI around it:
the entry points that refuse a walker handle, bad arguments, the stream contract of the new path through ddrl_env_step, the rollout
worker's unfused path with a learner update, and env.make / Wrapper."""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

VIT, PIT = 8, 3   # small counts keep the live oracle cheap; the kernel's loops are run-time counts, the same code as at 180 / 60
NAMES = ("obs2", "rew", "done", "next_obs", "ended")
NFW = 286


@pytest.fixture(scope="module")
def ddrl():
    import distributed_drl_amd as d
    d._lib.require_gpu()
    return d


def _vec(n, seed=0, max_ep_len=1600, vit=VIT, pit=PIT):
    from distributed_drl_amd.env import VecBipedalWalker
    return VecBipedalWalker(n, seed=seed, max_ep_len=max_ep_len, velocity_iterations=vit, position_iterations=pit)


def _oracle(n, seed=0, max_ep_len=1600, vit=VIT, pit=PIT):
    from walker_oracle import WalkerOracle
    return WalkerOracle(n, seed=seed, max_ep_len=max_ep_len, velocity_iterations=vit, position_iterations=pit)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# 64 / heuristic: gait contacts and the time limit; 33: not a multiple of a wave, actions beyond the torque clip; 1 / zero: motors at
# zero torque — the body collapses, the hull test fires, the reset is reached; 4096: 64 workgroups, and a time limit inside the run so
# that every lane goes through its reset.  What this matrix reaches and what it does not: profiles/walker_census.txt; the rest is held
# by the crafted states of tests/test_gpu_walker_scenarios.py.
@pytest.mark.parametrize("n,seed,policy,steps,max_len", [(64, 1, "heuristic", 300, 160), (33, 7, "random", 200, 1600),
                                                         (1, 3, "zero", 150, 1600), (4096, 11, "random", 20, 12)])
def test_walker_bit_exact_vs_live_oracle(ddrl, n, seed, policy, steps, max_len):
    from walker_oracle import WalkerHeuristic
    env, ora = _vec(n, seed, max_len), _oracle(n, seed, max_len)
    assert env.state_fields == NFW and (env.obs_dim, env.act_dim) == (24, 4)
    np.testing.assert_array_equal(env.obs.cpu().numpy(), ora.obs())
    np.testing.assert_array_equal(env.get_state().cpu().numpy(), ora.S)
    rs = np.random.RandomState(seed)
    ctl = WalkerHeuristic(n)
    o = ora.obs()
    n_ended = 0
    for t in range(steps):
        if policy == "heuristic":
            a = ctl.act(o)
        elif policy == "random":
            a = rs.uniform(-1.3, 1.3, (n, 4)).astype(np.float32)   # also exercises the torque clip
        else:
            a = np.zeros((n, 4), np.float32)
        g = [x.cpu().numpy() for x in env.step(_cuda(a))]
        w = ora.step(a)
        for name, gv, wv in zip(NAMES, g, w):
            np.testing.assert_array_equal(gv, wv, err_msg="%s at step %d" % (name, t))
        o = w[3]
        ctl.restart(w[4])
        n_ended += int(w[4].sum())
    np.testing.assert_array_equal(env.get_state().cpu().numpy(), ora.S)
    ge, gr, gl = env.stats()
    we, wr, wl = ora.stats()
    assert (ge, gl) == (we, wl) and ge == n_ended
    assert abs(gr - wr) <= 1e-9 * max(1.0, abs(wr))
    assert n_ended > 0
    if policy == "zero":
        assert ora.S[13, 0] >= 1.0   # the collapse ended an episode by the hull test: the reset was reached


def test_walker_bit_exact_vs_golden_file_at_gym_iterations(ddrl):
    """180 velocity / 60 position iterations, 8 envs: every recorded step and the final state block."""
    g = np.load(os.path.join(HERE, "golden", "walker_heuristic.npz"))
    n = int(g["n_envs"])
    env = _vec(n, int(g["seed"]), int(g["max_ep_len"]), vit=int(g["velocity_iterations"]), pit=int(g["position_iterations"]))
    outs = []
    for t in range(g["actions"].shape[0]):
        outs.append([x.clone() for x in env.step(_cuda(g["actions"][t]))])   # one host sync at the end
    for t, got in enumerate(outs):
        for name, idx in (("obs2", 0), ("rew", 1), ("done", 2), ("next_obs", 3), ("ended", 4)):
            np.testing.assert_array_equal(got[idx].cpu().numpy(), g[name][t], err_msg="%s at step %d" % (name, t))
    np.testing.assert_array_equal(env.get_state().cpu().numpy(), g["final_state"])
    ep, ret, ln = env.stats()
    assert ep == len(g["episode_return"]) and ln == int(g["episode_length"].sum())
    assert abs(ret - float(g["episode_return"].astype(np.float64).sum())) <= 1e-9 * max(1.0, abs(ret))


def test_walker_masked_reset_and_state_roundtrip(ddrl):
    env, ora = _vec(16, 5), _oracle(16, 5)
    a = np.tile(np.array([[0.7, -0.4, -0.6, 0.9]], np.float32), (16, 1))
    for _ in range(10):
        env.step(_cuda(a))
        ora.step(a)
    mask = (np.arange(16) % 3 == 0)
    g = env.reset(_cuda(mask.astype(np.uint8))).cpu().numpy()
    np.testing.assert_array_equal(g, ora.reset(mask))
    s = env.get_state()
    assert tuple(s.shape) == (NFW, 16)
    np.testing.assert_array_equal(s.cpu().numpy(), ora.S)
    env2 = _vec(16, 5)
    env2.set_state(s)
    g1 = [x.cpu().numpy() for x in env.step(_cuda(a))]
    g2 = [x.cpu().numpy() for x in env2.step(_cuda(a))]
    for name, x, y in zip(NAMES, g1, g2):
        np.testing.assert_array_equal(x, y, err_msg=name)
    np.testing.assert_array_equal(env.get_state().cpu().numpy(), env2.get_state().cpu().numpy())
    with pytest.raises(ValueError):
        env.set_state(torch.zeros(66, 16))   # the articulated lander's block size


def test_walker_time_limit_is_not_a_terminal(ddrl):
    """example/dsac.py:109,118: at ep_len == max_ep_len the stored done is 0 but the episode ends."""
    env = _vec(8, 0, max_ep_len=5)
    hold = torch.tensor([[0.1, 0.1, 0.1, 0.1]] * 8, device="cuda")
    for t in range(5):
        _, _, done, _, ended = env.step(hold)
        if t < 4:
            assert ended.sum().item() == 0
    assert done.sum().item() == 0 and ended.sum().item() == 8
    ep, _, ln = env.stats()
    assert (ep, ln) == (8, 40)


def _raw_create(lib, n, seed, max_ep_len, model):
    h = ctypes.c_void_p()
    rc = lib.ddrl_env_create_ex(ctypes.byref(h), torch.cuda.current_device(), n, seed, max_ep_len, None if model is None else ctypes.byref(model))
    return rc, h


def test_walker_bad_arguments(ddrl):
    """Iteration counts < 1 and kind 2 are refused at create; observation and action pointers off the 16-byte grid are refused by reset /
    step before any launch, with the state, the statistics and every output as they were."""
    from distributed_drl_amd import _lib
    from distributed_drl_amd.env import VecBipedalWalker
    lib = _lib.load()
    W = _lib.DDRL_ENV_WALKER
    assert W == 3 and _lib.DDRL_ENVW_STATE_FIELDS == NFW
    for model in (_lib.EnvModel(W, 0, 3), _lib.EnvModel(W, 8, 0), _lib.EnvModel(W, -1, -1), _lib.EnvModel(2, 8, 3), _lib.EnvModel(4, 8, 3)):
        rc, h = _raw_create(lib, 4, 0, 100, model)
        assert rc == _lib.DDRL_ERR_BAD_ARG and not h.value, (model.kind, model.velocity_iterations, model.position_iterations)
        assert lib.ddrl_last_error()
    with pytest.raises(ValueError):
        VecBipedalWalker(4, velocity_iterations=0)
    n = 8
    env = _vec(n, 2, 50)
    env.step(env.sample_actions())
    sp = _lib.stream_ptr()
    state0 = env.get_state().clone()
    SENT = 7.25
    pad = lambda *s: torch.full((int(np.prod(s)) + 4,), SENT, device="cuda")   # views at +1 float start 4 bytes off a 512-byte block
    good = lambda t, *s: t[4:4 + int(np.prod(s))].view(*s)
    off = lambda t, *s: t[1:1 + int(np.prod(s))].view(*s)
    bufs = {k: pad(*s) for k, s in (("act", (n, 4)), ("obs2", (n, 24)), ("next", (n, 24)), ("rew", (n,)), ("done", (n,)))}
    ended = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    bufs["act"][:] = 0.25

    def step(act, obs2, nxt):
        return lib.ddrl_env_step(env._h, _lib.dptr(act), _lib.dptr(obs2), _lib.dptr(good(bufs["rew"], n)), _lib.dptr(good(bufs["done"], n)),
                                 _lib.dptr(nxt), _lib.dptr(ended), sp)

    A, O, X = good(bufs["act"], n, 4), good(bufs["obs2"], n, 24), good(bufs["next"], n, 24)
    cases = {"act_d": lambda: step(off(bufs["act"], n, 4), O, X), "obs2_d": lambda: step(A, off(bufs["obs2"], n, 24), X),
             "next_obs_d": lambda: step(A, O, off(bufs["next"], n, 24)),
             "act_d (8-byte grid)": lambda: step(bufs["act"][2:2 + 4 * n].view(n, 4), O, X),
             "obs_d": lambda: lib.ddrl_env_reset(env._h, None, _lib.dptr(off(bufs["obs2"], n, 24)), sp)}
    for name, call in cases.items():
        assert call() == _lib.DDRL_ERR_BAD_ARG, name
        assert name.split(" ")[0].encode() in lib.ddrl_last_error(), (name, lib.ddrl_last_error())
        torch.cuda.synchronize()
        assert torch.equal(env.get_state(), state0), name
        for k in ("obs2", "next", "rew", "done"):
            assert bool((bufs[k] == SENT).all()), (name, k)
        assert bool((ended == 9).all()) and bool((bufs["act"] == 0.25).all()), name
    assert env.stats()[0] == 0
    assert step(A, O, X) == 0, lib.ddrl_last_error()   # the same call on the grid is taken
    torch.cuda.synchronize()
    assert not bool((O == SENT).any()) and not torch.equal(env.get_state(), state0)


class _Opt:
    obs_dim, act_dim, hidden_size, gamma, lr, polyak, batch_size, seed, alpha = 8, 4, [64, 48], 0.99, 1e-3, 0.995, 64, 3, 0.1
    num_envs, max_ep_len, start_steps, a_l_ratio, num_nodes, num_buffers, push_freq, buffer_size, variant = 32, 25, 0, 2, 1, 1, 50, 2048, "ddqn"


def _sac_opt(walker=False):
    from distributed_drl_amd.agent import HyperParameters
    opt = HyperParameters()
    opt.num_envs, opt.start_steps, opt.max_ep_len, opt.seed, opt.hidden_sizes = 32, -1, 25, 11, (64, 48)
    if walker:
        opt.env_model, opt.env_velocity_iterations, opt.env_position_iterations = "walker", VIT, PIT
        opt.obs_dim, opt.act_dim = 24, 4
    return opt


def test_refusing_entry_points_leave_everything_unchanged(ddrl):
    """Every entry point that takes an env handle, other than create / state_fields / reset / step / stats / get_state / set_state /
    destroy, on a walker handle: DDRL_ERR_UNSUPPORTED with its own name and "walker" in ddrl_last_error(), and the env state and
    observations, the caller's arrays, the actors (their weights, read through a deterministic forward of fixed rows), the rings
    (counters, cursor, rows) and the window queues as they were."""
    from distributed_drl_amd import _lib, dqn
    from distributed_drl_amd.agent import Actor
    from distributed_drl_amd.replay import ReplayBufferDQN
    from distributed_drl_amd.workers import WindowQueue
    lib = _lib.load()
    n = 32
    env = _vec(n, 4, 50)
    for _ in range(3):
        env.step(env.sample_actions())
    actor = Actor(_sac_opt(), max_rows=n)
    qactor = dqn.Actor(_Opt(), job="worker", max_rows=n)
    ring = ddrl.ReplayBufferSAC1(8, 2, 256, seed=0)
    qring = ReplayBufferDQN(_Opt(), 0, seed=5)
    winq = WindowQueue(n, 4, 8, 2)
    for rb, width in ((ring, 2), (qring, None)):   # some rows, so that "unchanged" is not "still empty"
        acts = torch.rand(40, 2, device="cuda") if width else torch.floor(torch.rand(40, device="cuda") * 4)
        rb.store_batch(torch.rand(40, 8, device="cuda"), acts, torch.rand(40, device="cuda"), torch.rand(40, 8, device="cuda"), torch.zeros(40, device="cuda"))
    probe = torch.rand(n, 8, device="cuda")
    act = torch.rand(n, 4, device="cuda")
    idx = torch.floor(torch.rand(n, device="cuda") * 4)
    out = [torch.full((n, 24), 3.5, device="cuda"), torch.full((n,), 3.5, device="cuda"), torch.full((n,), 3.5, device="cuda"),
           torch.full((n, 24), 3.5, device="cuda"), torch.full((n,), 5, dtype=torch.uint8, device="cuda")]

    def snapshot():
        torch.cuda.synchronize()
        snap = [env.get_state().clone(), env.obs.clone(), actor.get_actions(probe, deterministic=True).clone(), act.clone(), idx.clone()]
        snap += [x.clone() for x in out]
        q = torch.empty(n, 4, device="cuda")
        qactor.get_actions(probe, q_out=q, deterministic=True)
        snap.append(q)
        for rb in (ring, qring):
            snap.append(torch.tensor(list(rb.get_counts()) + [rb.ptr]))
            snap += [v.clone() for _, v in sorted(rb.rings().items())]
        snap += [x.clone() for x in winq.arrays]
        return snap

    sp = _lib.stream_ptr()
    o = [_lib.dptr(x) for x in out]
    ptrs = [ctypes.c_void_p() for _ in range(3)]
    dims = [ctypes.c_int32(-1), ctypes.c_int32(-1)]
    E, A, Q = env._h, actor._h, qactor._h
    calls = {
        "ddrl_env_step_discrete": lambda: lib.ddrl_env_step_discrete(E, _lib.dptr(idx), *o, sp),
        "ddrl_env_step_wrapped": lambda: lib.ddrl_env_step_wrapped(E, _lib.dptr(act), 0.3, 0.01, 5.0, 2, 100, *o, sp),
        "ddrl_env_step_wrapped_articulated": lambda: lib.ddrl_env_step_wrapped_articulated(E, _lib.dptr(act), 0.3, 0.01, 5.0, 2, 100, *o, sp),
        "ddrl_rollout_begin": lambda: lib.ddrl_rollout_begin(E, A, sp),
        "ddrl_rollout_step": lambda: lib.ddrl_rollout_step(E, A, ring._h, 1, 1, 0, 0, None, None, sp),
        "ddrl_rollout_begin_articulated": lambda: lib.ddrl_rollout_begin_articulated(E, A, sp),
        "ddrl_rollout_step_articulated": lambda: lib.ddrl_rollout_step_articulated(E, A, ring._h, 1, 1, 0, 0, None, None, sp),
        "ddrl_rollout_begin_discrete": lambda: lib.ddrl_rollout_begin_discrete(E, Q, sp),
        "ddrl_rollout_step_discrete": lambda: lib.ddrl_rollout_step_discrete(E, Q, qring._h, 1, _lib.DDRL_ACT_SAMPLE, 0.9, 1, 0, None, None, None, sp),
        "ddrl_rollout_begin_discrete_articulated": lambda: lib.ddrl_rollout_begin_discrete_articulated(E, Q, sp),
        "ddrl_rollout_step_discrete_articulated": lambda: lib.ddrl_rollout_step_discrete_articulated(E, Q, qring._h, 1, 0, 0.5, 1, 0, sp),
        "ddrl_rollout_begin_nstep": lambda: lib.ddrl_rollout_begin_nstep(E, A, winq._h, sp),
        "ddrl_rollout_step_nstep": lambda: lib.ddrl_rollout_step_nstep(E, A, winq._h, ring._h, 1, 0.3, 0.01, 5.0, 3, 100, 1, 7, 0, None, sp),
        "ddrl_rollout_begin_nstep_articulated": lambda: lib.ddrl_rollout_begin_nstep_articulated(E, A, winq._h, sp),
        "ddrl_rollout_step_nstep_articulated": lambda: lib.ddrl_rollout_step_nstep_articulated(E, A, winq._h, ring._h, 1, 0.3, 0.01, 5.0, 3, 100,
                                                                                            1, 7, 0, None, sp),
        "ddrl_env_eval_policy": lambda: lib.ddrl_env_eval_policy(E, A, 2, 0, 1, sp),
        "ddrl_env_eval_q": lambda: lib.ddrl_env_eval_q(E, Q, 2, 0, _lib.DDRL_ACT_SAMPLE, 0.5, 1, 0, 1, sp),
        "ddrl_env_rollout_mirrors": lambda: lib.ddrl_env_rollout_mirrors(E, *[ctypes.byref(x) for x in ptrs + dims]),
    }
    assert len(calls) == 18
    before = snapshot()
    for name, call in calls.items():
        assert call() == _lib.DDRL_ERR_UNSUPPORTED, (name, lib.ddrl_last_error())
        msg = lib.ddrl_last_error().decode()
        assert msg.startswith(name + ":") and "walker" in msg, (name, msg)
        after = snapshot()
        assert len(after) == len(before)
        for k, (x, y) in enumerate(zip(before, after)):
            assert torch.equal(x, y), (name, k)
    assert all(p.value is None for p in ptrs) and all(d.value == -1 for d in dims)
    # the results block of an evaluation was never made, and the env still steps
    rc = lib.ddrl_env_eval_results(E, *[ctypes.byref(x) for x in [ctypes.c_void_p() for _ in range(3)] + [ctypes.c_int32() for _ in range(3)]])
    assert rc == _lib.DDRL_ERR_BAD_ARG
    with pytest.raises(_lib.DdrlUnsupported, match="walker"):
        env.step_wrapped(act[:, :2].contiguous())
    env.step(act)
    assert not torch.equal(env.get_state(), before[0])


def test_walker_step_runs_on_the_callers_stream(ddrl):
    """The stream contract on the new path through ddrl_env_step: on a side stream, behind a bounded gate, the true actions are written
    over decoys and the step is issued.  A launch that went anywhere but the caller's stream would run during the gate, read the
    decoys and differ from the twin stepped with the true actions."""
    from _abi_arena import cycles_per_ms, side_stream
    n = 64
    env, twin = _vec(n, 21, 40), _vec(n, 21, 40)
    true = twin.sample_actions().clone()
    want = [x.clone() for x in twin.step(true)]
    want_state = twin.get_state().clone()
    dev = env.device
    act = torch.zeros(n, 4, device="cuda")        # the decoy: zero torque on every motor
    side = side_stream(dev)
    gate_end = torch.cuda.Event()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        torch.cuda._sleep(int(cycles_per_ms(dev) * 20.0))   # the gate: bounded, 20 ms
        gate_end.record()
        act.copy_(true)                                      # the late write
        got = env.step(act)
        issued_inside = not gate_end.query()
    side.synchronize()                                       # the caller's stream only, not the device
    got = [x.clone() for x in got]
    assert issued_inside, "the gate was over before the step was issued: the run proves nothing"
    for name, x, y in zip(NAMES, got, want):
        assert torch.equal(x, y), name
    assert torch.equal(env.get_state(), want_state)


def test_rollout_device_on_the_walker_runs_unfused_and_feeds_a_learner(ddrl):
    from distributed_drl_amd import _lib
    from distributed_drl_amd.agent import Learner
    from distributed_drl_amd.workers import RolloutDevice, RolloutDeviceDQN, RolloutDeviceNStep
    opt = _sac_opt(walker=True)
    learner = Learner(opt)
    assert (learner.cfg.obs_dim, learner.cfg.act_dim) == (24, 4)
    ps = ddrl.ParameterServer(*learner.get_weights())
    rb = ddrl.ReplayBufferSAC1(24, 4, 2048, seed=0)
    opt.obs_dim, opt.act_dim = 8, 2            # the worker sets them from the model
    roll = RolloutDevice(ps, rb, opt)
    assert (opt.obs_dim, opt.act_dim) == (24, 4) and tuple(roll.act.shape) == (32, 4) and tuple(roll.env.obs.shape) == (32, 24)
    n, steps, seen = roll.env.n, 40, []
    for _ in range(steps):
        roll.step()
        seen.append([x.clone() for x in (roll.o, roll.act, roll.env.obs2, roll.env.rew, roll.env.done)])
    assert roll._fused is False and roll.env.model == "walker" and roll.t == steps
    rings = rb.rings()
    for t, (o1, a, o2, r, d) in enumerate(seen):
        rows = slice(t * n, (t + 1) * n)
        assert torch.equal(rings["obs1_buf"][rows], o1), t
        assert torch.equal(rings["acts_buf"][rows], a), t
        assert torch.equal(rings["obs2_buf"][rows], o2), t
        assert torch.equal(rings["rews_buf"][rows].view(-1), r), t
        assert torch.equal(rings["done_buf"][rows].view(-1), d), t
    assert rb.get_counts()[1:] == (steps * n, steps * n)
    assert roll.env.stats()[0] >= n   # max_ep_len 25 < 40 steps: every env ended an episode on the way
    losses, _ = learner.train(rb.sample_batch_device(opt.batch_size), return_outputs=True)
    vals = np.array([float(v) for v in (losses.values() if isinstance(losses, dict) else losses)])
    assert len(vals) >= 2 and np.isfinite(vals).all(), losses
    assert learner._lib.ddrl_sac1_is_fused(learner._h) == 0   # obs + act = 28: the generic launch path
    for cls, args in ((RolloutDeviceDQN, (ps, rb, opt)), (RolloutDeviceNStep, (ps, [rb], opt))):
        with pytest.raises(ValueError, match="walker"):
            cls(*args)


def test_make_and_wrapper(ddrl):
    from distributed_drl_amd import env as E
    e = E.make("BipedalWalker-v2", model="walker", seed=2, max_ep_len=50, velocity_iterations=VIT, position_iterations=PIT)
    assert isinstance(e, E.BipedalWalker) and e._vec.state_fields == NFW
    assert e.observation_space.shape == (24,) and e.action_space.shape == (4,)
    s = e.action_space.sample()
    assert s.shape == (4,) and (np.abs(s) <= 1).all()
    ora = _oracle(1, 2, 50)
    o = e.reset()
    assert o.shape == (24,) and o.dtype == np.float64
    np.testing.assert_array_equal(o.astype(np.float32), ora.obs()[0])
    rs = np.random.RandomState(0)
    for t in range(12):
        a = rs.uniform(-1, 1, 4)
        o2, r, d, _ = e.step(a)
        w = ora.step(a.astype(np.float32)[None])
        np.testing.assert_array_equal(o2.astype(np.float32), w[0][0], err_msg="step %d" % t)
        assert r == float(w[1][0]) and d == bool(w[4][0])
    # the reference's Wrapper (hyperparams.py:107-134) with its 24 / 4 noise, unchanged
    w = E.Wrapper(e, obs_noise=0.01, act_noise=0.3, reward_scale=5.0, action_repeat=3, rng=np.random.RandomState(1))
    assert w.reset().shape == (24,)
    a = np.array([0.2, -0.1, 0.4, 0.3])
    a0 = a.copy()
    o2, r, d, _ = w.step(a)
    assert o2.shape == (24,) and np.isfinite(o2).all() and np.isfinite(r)
    assert not np.array_equal(a, a0) and (np.abs(a - a0) <= 0.3).all()   # `action +=`: the caller's 4-vector is changed in place
    # doors that stay shut
    for name, kw in (("BipedalWalkerHardcore-v2", dict(model="walker")), ("BipedalWalker-v2", dict()), ("BipedalWalker-v3", dict(model="walker")),
                     ("LunarLanderContinuous-v2", dict(model="walker"))):
        with pytest.raises(ValueError):
            E.make(name, **kw)
    with pytest.raises(ValueError, match="evaluation kernel"):
        E.make("BipedalWalker-v2", model="walker", on_device=True)
    with pytest.raises(ValueError, match="evaluation kernel"):
        E.make_device("BipedalWalker-v2", model="walker")
