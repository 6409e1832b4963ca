"""GPU parity of the ARTICULATED lander (ddrl_env_create_ex, kind = DDRL_ENV_ARTICULATED; csrc/env3_device.h) vs its specification
tests/lander3_oracle.py — BIT-EXACT, live at 8 / 3 iterations and against the golden file at gym's 180 / 60 — plus the C-ABI around
it: the one-body model untouched, the entry points that refuse an articulated handle, bad arguments, and the rollout workers' unfused
path on the new model."""
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


@pytest.fixture(scope="module")
def ddrl():
    import distributed_drl_amd as d
    d._lib.require_gpu()
    return d


def _heuristic(s):
    """gym's lunar_lander heuristic controller (a copy of tests/test_gpu_env.py's)."""
    angle_targ = np.clip(s[:, 0] * 0.5 + s[:, 2] * 1.0, -0.4, 0.4)
    hover_targ = 0.55 * np.abs(s[:, 0])
    angle_todo = (angle_targ - s[:, 4]) * 0.5 - s[:, 5] * 1.0
    hover_todo = (hover_targ - s[:, 1]) * 0.5 - s[:, 3] * 0.5
    legs = (s[:, 6] > 0) | (s[:, 7] > 0)
    angle_todo = np.where(legs, 0, angle_todo)
    hover_todo = np.where(legs, -s[:, 3] * 0.5, hover_todo)
    return np.clip(np.stack([hover_todo * 20 - 1, -angle_todo * 20], 1), -1, 1).astype(np.float32)


def _vec(n, seed=0, max_ep_len=1000, cls=None, vit=VIT, pit=PIT):
    from distributed_drl_amd.env import VecLunarLander
    return (cls or VecLunarLander)(n, seed=seed, max_ep_len=max_ep_len, model="articulated", velocity_iterations=vit, position_iterations=pit)


def _oracle(n, seed=0, max_ep_len=1000, vit=VIT, pit=PIT):
    from lander3_oracle import Lander3Oracle
    return Lander3Oracle(n, seed=seed, max_ep_len=max_ep_len, velocity_iterations=vit, position_iterations=pit)


# 64 / heuristic: contacts and the time limit; 33: not a multiple of a wave; 1: one lane; 4096: 64 workgroups, and a time limit
# inside the run so that every lane goes through its reset (no crash can happen within 20 steps of the start height).
# What this matrix reaches (profiles/lander3_census.txt, first table): contact on the legs' bottom corners (the top ones in a handful
# of env-steps), the near side of both joint limits, crashes by the hull's bottom vertices, viewport exits, the time limit.  It
# never reaches rest: at 8 / 3 the SLEEP counter stays at 0, so neither the sleep test nor the +100 exit runs, and the far side of
# the joint limits, the hull's top vertices and sloped or clamped terrain segments are touched in single env-steps at most.  Those
# branches are held by the crafted states of tests/test_gpu_lander3_scenarios.py.
@pytest.mark.parametrize("n,seed,policy,steps,max_len", [(64, 1, "heuristic", 300, 160), (33, 7, "random", 200, 1000),
                                                         (1, 3, "zero", 150, 1000), (4096, 11, "random", 20, 12)])
def test_env3_bit_exact_vs_live_oracle(ddrl, n, seed, policy, steps, max_len):
    env, ora = _vec(n, seed, max_len), _oracle(n, seed, max_len)
    assert env.state_fields == 66
    np.testing.assert_array_equal(env.obs.cpu().numpy(), ora.obs())
    np.testing.assert_array_equal(env.get_state().cpu().numpy(), ora.S)
    rs = np.random.RandomState(seed)
    o = ora.obs()
    n_ended = 0
    for t in range(steps):
        if policy == "heuristic":
            a = _heuristic(o)
        elif policy == "random":
            a = rs.uniform(-1.3, 1.3, (n, 2)).astype(np.float32)   # also exercises the action clip
        else:
            a = np.zeros((n, 2), np.float32)
        g = [x.cpu().numpy() for x in env.step(torch.from_numpy(a).cuda())]
        w = ora.step(a)
        for name, gv, wv in zip(NAMES, g, w):
            np.testing.assert_array_equal(gv, wv, err_msg="%s at step %d" % (name, t))
        o = w[3]
        n_ended += int(w[4].sum())
    np.testing.assert_array_equal(env.get_state().cpu().numpy(), ora.S)
    ge, gr, gl = env.stats()
    we, wr, wl = ora.stats()
    assert (ge, gl) == (we, wl) and ge == n_ended
    assert abs(gr - wr) <= 1e-9 * max(1.0, abs(wr))
    if policy != "zero":
        assert n_ended > 0


def test_env3_bit_exact_vs_golden_file_at_gym_iterations(ddrl):
    """180 velocity / 60 position iterations, 8 envs: every recorded step and the final state block."""
    g = np.load(os.path.join(HERE, "golden", "lander3_heuristic.npz"))
    n = int(g["n_envs"])
    env = _vec(n, int(g["seed"]), int(g["max_ep_len"]), vit=int(g["velocity_iterations"]), pit=int(g["position_iterations"]))
    outs = []
    for t in range(g["actions"].shape[0]):
        outs.append([x.clone() for x in env.step(torch.from_numpy(g["actions"][t]).cuda())])   # one host sync at the end
    for t, got in enumerate(outs):
        for name, idx in (("obs2", 0), ("rew", 1), ("done", 2), ("ended", 4)):
            np.testing.assert_array_equal(got[idx].cpu().numpy(), g[name][t], err_msg="%s at step %d" % (name, t))
    np.testing.assert_array_equal(env.get_state().cpu().numpy(), g["final_state"])
    ep, ret, ln = env.stats()
    assert ep == len(g["episode_return"]) and ln == int(g["episode_length"].sum())
    assert abs(ret - float(g["episode_return"].astype(np.float64).sum())) <= 1e-9 * abs(ret)


def test_env3_masked_reset_and_state_roundtrip(ddrl):
    env, ora = _vec(16, 5), _oracle(16, 5)
    a = np.full((16, 2), 0.7, np.float32)
    for _ in range(10):
        env.step(torch.from_numpy(a).cuda())
        ora.step(a)
    mask = (np.arange(16) % 3 == 0)
    g = env.reset(torch.from_numpy(mask.astype(np.uint8)).cuda()).cpu().numpy()
    np.testing.assert_array_equal(g, ora.reset(mask))
    s = env.get_state()
    assert tuple(s.shape) == (66, 16)
    np.testing.assert_array_equal(s.cpu().numpy(), ora.S)
    env2 = _vec(16, 5)
    env2.set_state(s)
    g1 = [x.cpu().numpy() for x in env.step(torch.from_numpy(a).cuda())]
    g2 = [x.cpu().numpy() for x in env2.step(torch.from_numpy(a).cuda())]
    for name, x, y in zip(NAMES, g1, g2):
        np.testing.assert_array_equal(x, y, err_msg=name)
    np.testing.assert_array_equal(env.get_state().cpu().numpy(), env2.get_state().cpu().numpy())
    with pytest.raises(ValueError):
        env.set_state(torch.zeros(32, 16))   # the one-body block size


def test_env3_time_limit_is_not_a_terminal(ddrl):
    """example/dsac.py:109,118: at ep_len == max_ep_len the stored done is 0 but the episode ends."""
    env = _vec(8, 0, max_ep_len=5)
    hover = torch.tensor([[0.3, 0.0]] * 8, device="cuda")
    for t in range(5):
        _, _, done, _, ended = env.step(hover)
        if t < 4:
            assert ended.sum().item() == 0
    assert done.sum().item() == 0 and ended.sum().item() == 8
    ep, _, ln = env.stats()
    assert (ep, ln) == (8, 40)


def test_env3_discrete_step_equals_the_tables_continuous_action(ddrl):
    """step_discrete with index k == step with the table's continuous action, bit for bit (index = (int)value clamped to [0, 3])."""
    from distributed_drl_amd.env import VecLunarLanderDiscrete
    table = np.array([[0.0, 0.0], [0.0, -1.0], [1.0, 0.0], [0.0, 1.0]], np.float32)
    n = 96
    dis, con = _vec(n, 9, 60, cls=VecLunarLanderDiscrete), _vec(n, 9, 60)
    rs = np.random.RandomState(2)
    ended = 0
    for t in range(90):
        idx = rs.randint(0, 4, n)
        gd = [x.cpu().numpy() for x in dis.step(torch.from_numpy(idx.astype(np.float32)).cuda())]
        gc = [x.cpu().numpy() for x in con.step(torch.from_numpy(table[idx]).cuda())]
        for name, x, y in zip(NAMES, gd, gc):
            np.testing.assert_array_equal(x, y, err_msg="%s at step %d" % (name, t))
        ended += int(gd[4].sum())
    np.testing.assert_array_equal(dis.get_state().cpu().numpy(), con.get_state().cpu().numpy())
    assert ended >= n


def _raw_create(lib, n, seed, max_ep_len, model):
    h = ctypes.c_void_p()
    rc = lib.ddrl_env_create_ex(ctypes.byref(h), torch.cuda.current_device(), n, seed, max_ep_len, None if model is None else ctypes.byref(model))
    return rc, h


def test_one_body_model_is_untouched(ddrl):
    """ddrl_env_state_fields is 32 on a ddrl_env_create handle; create_ex(kind = 0) — whatever its iteration fields — and
    create_ex(NULL) are that env bit for bit over 50 random steps."""
    from distributed_drl_amd import _lib
    from distributed_drl_amd.env import VecLunarLander
    lib = _lib.load()
    n = 200
    base = VecLunarLander(n, seed=13, max_ep_len=30)
    assert lib.ddrl_env_state_fields(base._h) == 32 and base.state_fields == 32 and base.model == "simple"
    handles = []
    for model in (_lib.EnvModel(_lib.DDRL_ENV_ONE_BODY, -7, 0), None):
        rc, h = _raw_create(lib, n, 13, 30, model)
        assert rc == 0 and lib.ddrl_env_state_fields(h) == 32
        handles.append(h)
    e = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device="cuda")
    bufs = [(e(n, 8), e(n), e(n), e(n, 8), e(n, dt=torch.uint8)) for _ in handles]
    states = [e(32, n) for _ in handles]
    rs = np.random.RandomState(0)
    ended = 0
    try:
        for t in range(50):
            a = torch.from_numpy(rs.uniform(-1.3, 1.3, (n, 2)).astype(np.float32)).cuda()
            want = [x.clone() for x in base.step(a)]
            for h, b in zip(handles, bufs):
                _lib.check(lib.ddrl_env_step(h, _lib.dptr(a), *[_lib.dptr(x) for x in b], _lib.stream_ptr()))
                for name, x, y in zip(NAMES, b, want):
                    assert torch.equal(x, y), "%s at step %d" % (name, t)
            ended += int(want[4].sum().item())
        for h, s in zip(handles, states):
            _lib.check(lib.ddrl_env_get_state(h, _lib.dptr(s), _lib.stream_ptr()))
            assert torch.equal(s, base.get_state())
    finally:
        for h in handles:
            lib.ddrl_env_destroy(h)
    assert ended >= n   # the 30-step limit: every env went through its reset


def test_bad_model_arguments(ddrl):
    from distributed_drl_amd import _lib
    from distributed_drl_amd.env import VecLunarLander
    lib = _lib.load()
    for model in (_lib.EnvModel(_lib.DDRL_ENV_ARTICULATED, 0, 3), _lib.EnvModel(_lib.DDRL_ENV_ARTICULATED, 8, 0),
                  _lib.EnvModel(_lib.DDRL_ENV_ARTICULATED, -1, -1), _lib.EnvModel(2, 8, 3), _lib.EnvModel(-1, 8, 3)):
        rc, h = _raw_create(lib, 4, 0, 100, model)
        assert rc == _lib.DDRL_ERR_BAD_ARG and not h.value, (model.kind, model.velocity_iterations, model.position_iterations)
        assert lib.ddrl_last_error()
    with pytest.raises(ValueError):
        VecLunarLander(4, model="articulated", velocity_iterations=0)
    with pytest.raises(ValueError):
        VecLunarLander(4, model="three-body")


def test_make_passes_the_model_on_and_refuses_on_device(ddrl):
    from distributed_drl_amd import env as E
    e = E.make("LunarLanderContinuous-v2", seed=2, max_ep_len=50, model="articulated", velocity_iterations=VIT, position_iterations=PIT)
    assert e._vec.model == "articulated" and e._vec.state_fields == 66
    o = e.reset()
    assert o.shape == (8,) and o.dtype == np.float64
    o2, r, d, _ = e.step(np.array([0.0, 0.0]))
    ora = _oracle(1, 2, 50)
    w = ora.step(np.zeros((1, 2), np.float32))
    np.testing.assert_array_equal(o2.astype(np.float32), w[0][0])
    assert r == float(w[1][0])
    d2 = E.make("LunarLander-v2", seed=2, max_ep_len=50, model="articulated", velocity_iterations=VIT, position_iterations=PIT)
    assert d2._vec.model == "articulated" and d2.action_space.n == 4
    assert E.make("LunarLanderContinuous-v2", seed=2)._vec.model == "simple"
    for name in ("LunarLanderContinuous-v2", "LunarLander-v2"):
        with pytest.raises(ValueError, match="evaluation kernel"):
            E.make(name, on_device=True, model="articulated")
    assert E.make("LunarLanderContinuous-v2", on_device=True, model="simple").on_device


class _Opt:
    obs_dim, act_dim, hidden_size, gamma, lr, polyak, batch_size, seed, alpha = 8, 4, [64, 48], 0.99, 1e-3, 0.995, 64, 3, 0.1
    num_envs, max_ep_len, start_steps, a_l_ratio, num_nodes, num_buffers, push_freq, buffer_size, variant = 32, 25, 0, 2, 1, 1, 50, 2048, "ddqn"
    env_model, env_velocity_iterations, env_position_iterations = "articulated", VIT, PIT


def _sac_opt():
    from distributed_drl_amd.agent import HyperParameters
    opt = HyperParameters()
    opt.num_envs, opt.start_steps, opt.max_ep_len, opt.seed, opt.hidden_sizes = 32, -1, 25, 11, (64, 48)
    opt.env_model, opt.env_velocity_iterations, opt.env_position_iterations = "articulated", VIT, PIT
    return opt


def test_refusing_entry_points_leave_everything_unchanged(ddrl):
    """ddrl_env_step_wrapped, ddrl_rollout_begin / _step and ddrl_rollout_begin_discrete / _step_discrete on an articulated handle:
    DDRL_ERR_UNSUPPORTED with a reason, and the env state and observations, the actors (their weights, read through a deterministic
    forward of fixed rows), the caller's action array and the rings (counters, cursor, rows) as they were."""
    from distributed_drl_amd import _lib, dqn
    from distributed_drl_amd.agent import Actor
    from distributed_drl_amd.replay import ReplayBufferDQN
    lib = _lib.load()
    n = 32
    env = _vec(n, 4, 50)
    for _ in range(3):
        env.step(env.sample_actions())
    opt = _sac_opt()
    actor = Actor(opt, max_rows=n)
    qactor = dqn.Actor(_Opt(), job="worker", max_rows=n)
    ring = ddrl.ReplayBufferSAC1(8, 2, 256, seed=0)
    qring = ReplayBufferDQN(_Opt(), 0, seed=5)
    for rb, width in ((ring, 2), (qring, None)):   # some rows, so that "unchanged" is not "still empty"
        acts = torch.rand(40, 2, device="cuda") if width else torch.floor(torch.rand(40, device="cuda") * 4)
        rb.store_batch(torch.rand(40, 8, device="cuda"), acts, torch.rand(40, device="cuda"), torch.rand(40, 8, device="cuda"), torch.zeros(40, device="cuda"))
    probe = torch.rand(n, 8, device="cuda")

    def snapshot():
        torch.cuda.synchronize()
        snap = [env.get_state().clone(), env.obs.clone(), actor.get_actions(probe, deterministic=True).clone()]
        q = torch.empty(n, 4, device="cuda")
        qactor.get_actions(probe, q_out=q, deterministic=True)
        snap.append(q)
        for rb in (ring, qring):
            snap.append(torch.tensor(list(rb.get_counts()) + [rb.ptr]))
            snap += [v.clone() for _, v in sorted(rb.rings().items())]
        return snap

    act = torch.rand(n, 2, device="cuda")
    act0 = act.clone()
    out = [torch.empty(n, 8, device="cuda"), torch.empty(n, device="cuda"), torch.empty(n, device="cuda"), torch.empty(n, 8, device="cuda"),
           torch.empty(n, dtype=torch.uint8, device="cuda")]
    sp = _lib.stream_ptr()
    calls = {
        "ddrl_env_step_wrapped": lambda: lib.ddrl_env_step_wrapped(env._h, _lib.dptr(act), 0.3, 0.01, 5.0, 2, 100, *[_lib.dptr(x) for x in out], sp),
        "ddrl_rollout_begin": lambda: lib.ddrl_rollout_begin(env._h, actor._h, sp),
        "ddrl_rollout_step": lambda: lib.ddrl_rollout_step(env._h, actor._h, ring._h, 1, 1, 0, 0, None, None, sp),
        "ddrl_rollout_begin_discrete": lambda: lib.ddrl_rollout_begin_discrete(env._h, qactor._h, sp),
        "ddrl_rollout_step_discrete": lambda: lib.ddrl_rollout_step_discrete(env._h, qactor._h, qring._h, 1, _lib.DDRL_ACT_SAMPLE, 0.9, 1, 0, None, None,
                                                                            None, sp),
    }
    before = snapshot()
    for name, call in calls.items():
        assert call() == _lib.DDRL_ERR_UNSUPPORTED, name
        msg = lib.ddrl_last_error().decode()
        assert name in msg and "articulated" in msg, (name, msg)
        after = snapshot()
        assert len(after) == len(before)
        for k, (x, y) in enumerate(zip(before, after)):
            assert torch.equal(x, y), (name, k)
        assert torch.equal(act, act0), name
    # the same calls are taken by a one-body env of the same shape (the refusal is the model's, not the arguments')
    from distributed_drl_amd.env import VecLunarLander
    plain = VecLunarLander(n, seed=4, max_ep_len=50)
    assert lib.ddrl_rollout_begin(plain._h, actor._h, sp) == 0
    assert lib.ddrl_rollout_begin_discrete(plain._h, qactor._h, sp) == 0
    with pytest.raises(_lib.DdrlUnsupported):
        env.step_wrapped(act)


def _check_ring_rows_are_the_envs_transitions(roll, rb, steps):
    n = roll.env.n
    seen = []
    for _ in range(steps):
        roll.step()
        seen.append([x.clone() for x in (roll.env.obs2, roll.env.rew, roll.env.done)])
    assert roll._fused is False and roll.env.model == "articulated"
    rings = rb.rings()
    for t, (o2, r, d) in enumerate(seen):
        rows = slice(t * n, (t + 1) * n)
        assert torch.equal(rings["obs2_buf"][rows], o2), t
        assert torch.equal(rings["rews_buf"][rows].view(-1), r), t
        assert torch.equal(rings["done_buf"][rows].view(-1), d), t
    assert rb.get_counts()[1:] == (steps * n, steps * n)
    assert roll.env.stats()[0] >= n   # max_ep_len 25 < 40 steps: every env ended an episode on the way


def test_rollout_device_on_the_articulated_model_runs_unfused(ddrl):
    from distributed_drl_amd.agent import Learner
    from distributed_drl_amd.workers import RolloutDevice
    opt = _sac_opt()
    ps = ddrl.ParameterServer(*Learner(opt).get_weights())
    rb = ddrl.ReplayBufferSAC1(8, 2, 2048, seed=0)
    roll = RolloutDevice(ps, rb, opt)
    _check_ring_rows_are_the_envs_transitions(roll, rb, 40)
    assert roll.t == 40


def test_rollout_device_dqn_on_the_articulated_model_runs_unfused(ddrl):
    from distributed_drl_amd import dqn
    from distributed_drl_amd.ps import ParameterServer
    from distributed_drl_amd.replay import ReplayBufferDQN
    from distributed_drl_amd.workers import RolloutDeviceDQN
    opt = _Opt()
    ps = ParameterServer(*dqn.Learner(opt).get_weights())
    rb = ReplayBufferDQN(opt, 0, seed=5)
    roll = RolloutDeviceDQN(ps, rb, opt)
    _check_ring_rows_are_the_envs_transitions(roll, rb, 40)
    assert roll.t == 40 * 32
    assert set(rb.rings()["acts_buf"][:40 * 32].view(-1).cpu().numpy().tolist()) <= {0.0, 1.0, 2.0, 3.0}
