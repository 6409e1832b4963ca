"""GPU parity of the walker on the HARDCORE terrain (ddrl_env_create_walker, include/ddrl_walker_hardcore.h; csrc/walker.hip
over csrc/walker_device.h's WalkerT<1>) vs its specification tests/walker_hardcore_oracle.py — BIT-EXACT, live at 8 / 3 iterations: the
plain step, the wrapped step against the reused wrapped oracle — plus the C-ABI around it: the grass door, the block size, the refusals
(with everything left as it was), the rollout workers' unfused sequences with a learner update, and env.make / Wrapper.
The crafted obstacle states: tests/test_gpu_walker_hardcore_scenarios.py."""
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
NFW, NFWH = 286, 663


@pytest.fixture(scope="module")
def ddrl():
    import distributed_drl_amd as d
    d._lib.require_gpu()
    torch.cuda.set_device(0)
    return d


def _vec(n, seed=0, max_ep_len=1600, vit=VIT, pit=PIT, terrain="hardcore"):
    from distributed_drl_amd.env import VecBipedalWalker
    return VecBipedalWalker(n, seed=seed, max_ep_len=max_ep_len, velocity_iterations=vit, position_iterations=pit, terrain=terrain)


def _oracle(n, seed=0, max_ep_len=1600, vit=VIT, pit=PIT, cls="WalkerHardcoreOracle"):
    import walker_hardcore_oracle as H
    return getattr(H, cls)(n, seed=seed, max_ep_len=max_ep_len, velocity_iterations=vit, position_iterations=pit)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# 64 / limit 12: a full wave, five regenerated terrains per env; 33: a partial wave; 1 / zero: a collapse that reaches the reset through
# the hull test; 130 / limit 7: three workgroups with a tail
@pytest.mark.parametrize("n,seed,policy,steps,max_len", [(64, 1, "random", 60, 12), (33, 7, "random", 60, 1600), (1, 3, "zero", 150, 1600),
                                                         (130, 11, "random", 20, 7)])
def test_hardcore_bit_exact_vs_live_oracle(ddrl, n, seed, policy, steps, max_len):
    import walker_hardcore_oracle as H
    env, ora = _vec(n, seed, max_len), _oracle(n, seed, max_len)
    assert env.state_fields == NFWH == H.NFWH and (env.obs_dim, env.act_dim) == (24, 4) and env.terrain == "hardcore"
    np.testing.assert_array_equal(env.obs.cpu().numpy(), ora.obs())
    np.testing.assert_array_equal(env.get_state().cpu().numpy(), ora.S)
    assert (ora.S[H.NB] >= 3).all()            # every terrain holds obstacles: the box rows compared above are not empty
    rs = np.random.RandomState(seed)
    n_ended = 0
    outs = []
    for t in range(steps):
        a = rs.uniform(-1.3, 1.3, (n, 4)).astype(np.float32) if policy == "random" else np.zeros((n, 4), np.float32)
        outs.append(([x.clone() for x in env.step(_cuda(a))], ora.step(a)))
        n_ended += int(outs[-1][1][4].sum())
    for t, (g, w) in enumerate(outs):
        for name, gv, wv in zip(NAMES, g, w):
            np.testing.assert_array_equal(gv.cpu().numpy(), wv, err_msg="%s at step %d" % (name, t))
    np.testing.assert_array_equal(env.get_state().cpu().numpy(), ora.S)
    ge, gr, gl = env.stats()
    we, wr, wl = ora.stats()
    assert (ge, gl) == (we, wl) and ge == n_ended and n_ended > 0
    assert abs(gr - wr) <= 1e-9 * max(1.0, abs(wr))
    if policy == "zero":
        assert ora.S[13, 0] >= 1.0   # the collapse ended an episode by the hull test: the reset was reached


@pytest.mark.parametrize("repeat,obs_noise,limit", [(1, 0.05, 4), (2, 0.05, 3), (3, 0.0, 3), (3, 0.05, 50)])
def test_hardcore_wrapped_step_bit_exact_vs_the_reused_wrapped_oracle(ddrl, repeat, obs_noise, limit):
    """ddrl_env_step_wrapped_walker on a Hardcore handle vs WalkerWrappedOracle.step_wrapped on the Hardcore class: repeat 1, 2, 3,
    noise on and off, limits small enough that every env resets (terrain regenerated inside the launch); env 0 starts from a crafted
    state with the hull's nose inside a stump, so that a sub-step ends its episode at a box."""
    import _walker_hardcore_scenarios as sc
    import walker_hardcore_oracle as H
    n, seed = 40, 9
    env, ora = _vec(n, seed), _oracle(n, seed, cls="WalkerHardcoreWrappedOracle")
    S, _ = sc.build()
    e_src = sc.CLASSES.index("hull_in_box")
    blk = ora.S.copy()
    blk[:, 0] = S[:, e_src]
    blk[13, 0] = ora.S[13, 0]
    ora.S[:] = blk
    env.set_state(_cuda(blk))
    rs = np.random.RandomState(3)
    box_end = False
    for t in range(8):
        a = rs.uniform(-1.2, 1.2, (n, 4)).astype(np.float32)
        if t == 0:
            a[0] = 0.0
        ag, aw = _cuda(a.copy()), a.copy()
        g = [x.cpu().numpy() for x in env.step_wrapped_walker(ag, 0.3, obs_noise, 5.0, repeat, limit)]
        w = ora.step_wrapped(aw, 0.3, obs_noise, 5.0, repeat, limit)
        if t == 0:
            box_end = bool(ora.last["box_over"][0]) or bool(w[2][0])
        np.testing.assert_array_equal(ag.cpu().numpy(), aw, err_msg="noisy action at step %d" % t)
        for name, gv, wv in zip(NAMES, g, w):
            np.testing.assert_array_equal(gv, np.asarray(wv), err_msg="%s at step %d" % (name, t))
    np.testing.assert_array_equal(env.get_state().cpu().numpy(), ora.S)
    assert box_end                             # env 0's first wrapped step ended at the box
    ge, gr, gl = env.stats()
    we, wr, wl = ora.stats()
    assert (ge, gl) == (we, wl) and abs(gr - wr) <= 1e-9 * max(1.0, abs(wr))
    if limit < 8:
        assert (ora.S[13] >= 1.0).all()        # every env went through a reset


def _create_walker(lib, n, seed, max_ep_len, vit, pit, terrain):
    h = ctypes.c_void_p()
    rc = lib.ddrl_env_create_walker(ctypes.byref(h), torch.cuda.current_device(), n, seed, max_ep_len, vit, pit, terrain)
    return rc, h


def test_grass_door_is_the_grass_walker(ddrl):
    """ddrl_env_create_walker(terrain = GRASS) and ddrl_env_create_ex(kind = WALKER): equal outputs and equal 286-row blocks over 30
    steps with one seed — and VecBipedalWalker(terrain="grass") is the env it was."""
    from distributed_drl_amd import _lib
    lib = _lib.load()
    n, seed = 48, 5
    a_env = _vec(n, seed, 9, terrain="grass")
    assert a_env.state_fields == NFW and a_env.terrain == "grass"
    rc, h = _create_walker(lib, n, seed, 9, VIT, PIT, _lib.DDRL_WALKER_TERRAIN_GRASS)
    assert rc == 0 and lib.ddrl_env_state_fields(h) == NFW
    try:
        sp = _lib.stream_ptr()
        outs = [torch.empty(n, 24, device="cuda"), torch.empty(n, device="cuda"), torch.empty(n, device="cuda"), torch.empty(n, 24, device="cuda"),
                torch.empty(n, dtype=torch.uint8, device="cuda")]
        st = torch.empty(NFW, n, device="cuda")
        rs = np.random.RandomState(1)
        for t in range(30):
            a = _cuda(rs.uniform(-1.2, 1.2, (n, 4)).astype(np.float32))
            want = a_env.step(a)
            assert lib.ddrl_env_step(h, _lib.dptr(a), *[_lib.dptr(x) for x in outs], sp) == 0
            for name, x, y in zip(NAMES, outs, want):
                assert torch.equal(x, y), (name, t)
        assert lib.ddrl_env_get_state(h, _lib.dptr(st), sp) == 0
        assert torch.equal(st, a_env.get_state())
    finally:
        lib.ddrl_env_destroy(h)


def test_hardcore_masked_reset_and_state_roundtrip(ddrl):
    env, ora = _vec(16, 5), _oracle(16, 5)
    a = np.tile(np.array([[0.7, -0.4, -0.6, 0.9]], np.float32), (16, 1))
    for _ in range(6):
        env.step(_cuda(a))
        ora.step(a)
    mask = (np.arange(16) % 3 == 0)
    ora.S[13, mask] += 1.0                     # another episode number, so that the masked envs' terrains change
    blk = _cuda(ora.S)
    env.set_state(blk)
    g = env.reset(_cuda(mask.astype(np.uint8))).cpu().numpy()
    np.testing.assert_array_equal(g, ora.reset(mask))
    s = env.get_state()
    assert tuple(s.shape) == (NFWH, 16)
    np.testing.assert_array_equal(s.cpu().numpy(), ora.S)
    env2 = _vec(16, 99)
    env2.set_state(s)
    g1 = [x.cpu().numpy() for x in env.step(_cuda(a))]
    g2 = [x.cpu().numpy() for x in env2.step(_cuda(a))]
    for name, x, y in zip(NAMES, g1, g2):
        np.testing.assert_array_equal(x, y, err_msg=name)
    np.testing.assert_array_equal(env.get_state().cpu().numpy()[:, :], env2.get_state().cpu().numpy())
    grass = _vec(16, 5, terrain="grass")
    with pytest.raises(ValueError):
        env.set_state(torch.zeros(NFW, 16))    # the grass walker's block is refused by a Hardcore env ...
    with pytest.raises(ValueError):
        grass.set_state(torch.zeros(NFWH, 16))  # ... and the other way round


def _sac_opt():
    from distributed_drl_amd.agent import HyperParameters
    opt = HyperParameters()
    opt.num_envs, opt.start_steps, opt.max_ep_len, opt.seed, opt.hidden_sizes = 32, -1, 25, 11, (64, 48)
    opt.env_model, opt.env_velocity_iterations, opt.env_position_iterations, opt.env_terrain = "walker", VIT, PIT, "hardcore"
    opt.obs_dim, opt.act_dim = 24, 4
    return opt


def test_refusals_leave_everything_unchanged(ddrl):
    """Bad terrain values and iteration counts at create; ddrl_env_eval_policy_walker and three of the lander entry points on a Hardcore
    handle; pointers off the 16-byte grid at step / reset / step_wrapped_walker.  After each refused call the state block, the
    statistics and the caller's arrays are as they were."""
    import _abi_contract_walker_hardcore as ah
    from distributed_drl_amd import _lib
    from distributed_drl_amd.agent import Actor
    from distributed_drl_amd.env import DeviceBipedalWalker, VecBipedalWalker
    lib = _lib.load()
    for vit, pit, terrain in ((VIT, PIT, 2), (VIT, PIT, -1), (VIT, PIT, 7), (0, PIT, 1), (VIT, 0, 1), (-1, -1, 0)):
        h = ctypes.c_void_p()
        h.value = 0x1234                       # *out must stay untouched
        rc = lib.ddrl_env_create_walker(ctypes.byref(h), torch.cuda.current_device(), 4, 0, 100, vit, pit, terrain)
        assert rc == _lib.DDRL_ERR_BAD_ARG and h.value == 0x1234, (vit, pit, terrain)
        assert lib.ddrl_last_error()
    for bad in ("Hardcore", "stumps", None, 1):
        with pytest.raises(ValueError):
            VecBipedalWalker(4, terrain=bad)
    with pytest.raises(ValueError, match="evaluation kernel"):
        DeviceBipedalWalker(terrain="hardcore")
    n = 8
    env = _vec(n, 2, 50)
    env.step(env.sample_actions())
    sp = _lib.stream_ptr()
    opt = _sac_opt()
    actor = Actor(opt, max_rows=n)
    SENT = 7.25
    pad = lambda *s: torch.full((int(np.prod(s)) + 4,), SENT, device="cuda")   # views at +1 float start 4 bytes off the 16-byte grid
    good = lambda t, *s: t[4:4 + int(np.prod(s))].view(*s)
    off = lambda t, *s: t[1:1 + int(np.prod(s))].view(*s)
    bufs = {k: pad(*s) for k, s in (("act", (n, 4)), ("obs2", (n, 24)), ("next", (n, 24)), ("rew", (n,)), ("done", (n,)))}
    ended = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    bufs["act"][:] = 0.25
    idx = torch.zeros(n, device="cuda")

    def step(act, obs2, nxt):
        return lib.ddrl_env_step(env._h, _lib.dptr(act), _lib.dptr(obs2), _lib.dptr(good(bufs["rew"], n)), _lib.dptr(good(bufs["done"], n)),
                                 _lib.dptr(nxt), _lib.dptr(ended), sp)

    def wrapped(act, obs2, nxt):
        return lib.ddrl_env_step_wrapped_walker(env._h, _lib.dptr(act), 0.3, 0.01, 5.0, 2, 100, _lib.dptr(obs2), _lib.dptr(good(bufs["rew"], n)),
                                                _lib.dptr(good(bufs["done"], n)), _lib.dptr(nxt), _lib.dptr(ended), sp)

    A, O, X = good(bufs["act"], n, 4), good(bufs["obs2"], n, 24), good(bufs["next"], n, 24)
    o5 = [_lib.dptr(t) for t in (O, good(bufs["rew"], n), good(bufs["done"], n), X, ended)]
    BAD, UNS = _lib.DDRL_ERR_BAD_ARG, _lib.DDRL_ERR_UNSUPPORTED
    cases = [
        ("ddrl_env_step", "act_d", BAD, lambda: step(off(bufs["act"], n, 4), O, X)),
        ("ddrl_env_step", "obs2_d", BAD, lambda: step(A, off(bufs["obs2"], n, 24), X)),
        ("ddrl_env_step", "next_obs_d", BAD, lambda: step(A, O, off(bufs["next"], n, 24))),
        ("ddrl_env_reset", "obs_d", BAD, lambda: lib.ddrl_env_reset(env._h, None, _lib.dptr(off(bufs["obs2"], n, 24)), sp)),
        ("ddrl_env_step_wrapped_walker", "act_d", BAD, lambda: wrapped(off(bufs["act"], n, 4), O, X)),
        ("ddrl_env_step_wrapped_walker", "obs2_d", BAD, lambda: wrapped(A, off(bufs["obs2"], n, 24), X)),
        ("ddrl_env_step_wrapped_walker", "next_obs_d", BAD, lambda: wrapped(A, O, off(bufs["next"], n, 24))),
        ("ddrl_env_eval_policy_walker", "hardcore", UNS, lambda: lib.ddrl_env_eval_policy_walker(env._h, actor._h, 2, 0, 1, sp)),
        ("ddrl_env_step_discrete", "walker", UNS, lambda: lib.ddrl_env_step_discrete(env._h, _lib.dptr(idx), *o5, sp)),
        ("ddrl_env_step_wrapped", "walker", UNS, lambda: lib.ddrl_env_step_wrapped(env._h, _lib.dptr(A), 0.3, 0.01, 5.0, 2, 100, *o5, sp)),
        ("ddrl_env_eval_policy", "walker", UNS, lambda: lib.ddrl_env_eval_policy(env._h, actor._h, 2, 0, 1, sp)),
    ]
    assert [(f, p) for f, p, rc, _ in cases if rc == BAD] == ah.REFUSALS
    probe = torch.rand(n, 24, device="cuda")
    state0, obs0, pol0 = env.get_state().clone(), env.obs.clone(), actor.get_actions(probe, deterministic=True).clone()
    for fn, word, want, call in cases:
        assert call() == want, (fn, word, lib.ddrl_last_error())
        msg = lib.ddrl_last_error().decode()
        assert word in msg, (fn, word, msg)
        if want == UNS:
            assert msg.startswith(fn + ":"), msg
        torch.cuda.synchronize()
        assert torch.equal(env.get_state(), state0) and torch.equal(env.obs, obs0), (fn, word)
        for k in ("obs2", "next", "rew", "done"):
            assert bool((bufs[k] == SENT).all()), (fn, word, k)
        assert bool((ended == 9).all()) and bool((bufs["act"] == 0.25).all()) and bool((idx == 0).all()), (fn, word)
        assert torch.equal(actor.get_actions(probe, deterministic=True), pol0), (fn, word)
    assert env.stats()[0] == 0
    rc = lib.ddrl_env_eval_results(env._h, *[ctypes.byref(x) for x in [ctypes.c_void_p() for _ in range(3)] + [ctypes.c_int32() for _ in range(3)]])
    assert rc == BAD                            # no results block was made
    assert step(A, O, X) == 0, lib.ddrl_last_error()   # the same call on the grid is taken
    torch.cuda.synchronize()
    assert not bool((O == SENT).any()) and not torch.equal(env.get_state(), state0)


def test_rollout_workers_run_their_unfused_sequences_on_the_hardcore_terrain(ddrl):
    from distributed_drl_amd.agent import HyperParameters, Learner
    from distributed_drl_amd.workers import RolloutDevice, RolloutDeviceDQN, RolloutDeviceNStep, _default_test_env, _env_model_kw
    opt = _sac_opt()
    assert _env_model_kw(opt)["terrain"] == "hardcore"
    learner = Learner(opt)
    ps = ddrl.ParameterServer(*learner.get_weights())
    rb = ddrl.ReplayBufferSAC1(24, 4, 2048, seed=0)
    roll = RolloutDevice(ps, rb, opt)
    assert roll.env.terrain == "hardcore" and roll.env.state_fields == NFWH and tuple(roll.env.obs.shape) == (32, 24)
    n, steps, seen = roll.env.n, 40, []
    for _ in range(steps):
        roll.step()
        seen.append([x.clone() for x in (roll.o, roll.act, roll.env.obs2, roll.env.rew, roll.env.done)])
    assert roll._fused is False and roll.t == steps
    rings = rb.rings()
    for t, (o1, a, o2, r, d) in enumerate(seen):
        rows = slice(t * n, (t + 1) * n)
        assert torch.equal(rings["obs1_buf"][rows], o1), t
        assert torch.equal(rings["acts_buf"][rows], a), t
        assert torch.equal(rings["obs2_buf"][rows], o2), t
        assert torch.equal(rings["rews_buf"][rows].view(-1), r), t
        assert torch.equal(rings["done_buf"][rows].view(-1), d), t
    assert roll.env.stats()[0] >= n            # max_ep_len 25 < 40 steps: every env ended an episode on the way
    losses, _ = learner.train(rb.sample_batch_device(opt.batch_size), return_outputs=True)
    vals = np.array([float(v) for v in (losses.values() if isinstance(losses, dict) else losses)])
    assert len(vals) >= 2 and np.isfinite(vals).all(), losses
    with pytest.raises(ValueError, match="walker"):
        RolloutDeviceDQN(ps, rb, opt)
    # the n-step worker: 10 steps into a 24 / 4 window ring, against the env stepped by hand
    nopt = HyperParameters(obs_dim=24, act_dim=4)
    nopt.hidden_sizes = (64, 48)
    nopt.num_envs, nopt.seed, nopt.Ln, nopt.save_freq, nopt.start_steps = 32, 3, 3, 1, 100
    nopt.max_ep_len, nopt.action_repeat = 12, 2
    nopt.buffer_size, nopt.batch_size, nopt.num_buffers = 150, 8, 1
    nopt.obs_noise, nopt.act_noise, nopt.reward_scale = 0.01, 0.3, 5
    nopt.env_model, nopt.env_velocity_iterations, nopt.env_position_iterations, nopt.env_terrain = "walker", VIT, PIT, "hardcore"
    nlearner = Learner(nopt)
    nps = ddrl.ParameterServer(*nlearner.get_weights())
    nrb = ddrl.ReplayBufferNStep(nopt)
    ro = RolloutDeviceNStep(nps, nrb, nopt)
    assert ro.env.terrain == "hardcore" and ro.env.state_fields == NFWH and (ro.winq.obs_dim, ro.winq.act_dim) == (24, 4)
    twin = _vec(32, ro.env.seed, ro.env.max_ep_len)
    np.testing.assert_array_equal(twin.get_state().cpu().numpy(), ro.env.get_state().cpu().numpy())
    for s in range(10):
        ro.step()                              # start_steps 100: the actions are the env's own samples, which the twin draws alike
        act = twin.sample_actions()
        twin.step_wrapped_walker(act, nopt.act_noise, nopt.obs_noise, nopt.reward_scale, ro.WRAPPER_REPEAT, ro.limit_steps)
        assert torch.equal(ro.act, act) and torch.equal(ro.env.obs, twin.obs) and torch.equal(ro.env.get_state(), twin.get_state()), s
    assert ro._fused is not True and nrb._counts()[1] > 0
    losses, _ = nlearner.train(nrb.sample_batch(), return_outputs=True)
    v = np.array([float(x) for x in (losses.values() if isinstance(losses, dict) else losses)])
    assert len(v) >= 2 and np.isfinite(v).all(), losses
    # the test worker's env: the device marker refuses, the host loop's env (the default) is a lander as before
    opt.test_on_device = True
    with pytest.raises(ValueError, match="evaluation kernel"):
        _default_test_env("BipedalWalkerHardcore-v2", opt)
    bad = _sac_opt()
    bad.env_model = "articulated"
    with pytest.raises(ValueError, match="env_terrain"):
        _env_model_kw(bad)


def test_make_doors_and_wrapper(ddrl):
    from distributed_drl_amd import env as E
    kw = dict(seed=2, max_ep_len=50, velocity_iterations=VIT, position_iterations=PIT)
    e = E.make("BipedalWalkerHardcore-v2", model="walker", terrain="hardcore", **kw)
    assert isinstance(e, E.BipedalWalker) and e._vec.state_fields == NFWH and e._vec.terrain == "hardcore"
    ora = _oracle(1, 2, 50)
    o = e.reset()
    assert o.shape == (24,) and o.dtype == np.float64
    np.testing.assert_array_equal(o.astype(np.float32), ora.obs()[0])
    rs = np.random.RandomState(0)
    for t in range(8):
        a = rs.uniform(-1, 1, 4)
        o2, r, d, _ = e.step(a)
        w = ora.step(a.astype(np.float32)[None])
        np.testing.assert_array_equal(o2.astype(np.float32), w[0][0], err_msg="step %d" % t)
        assert r == float(w[1][0]) and d == bool(w[4][0])
    w = E.Wrapper(e, obs_noise=0.01, act_noise=0.3, reward_scale=5.0, action_repeat=3, rng=np.random.RandomState(1))
    assert w.reset().shape == (24,)
    o2, r, d, _ = w.step(np.array([0.2, -0.1, 0.4, 0.3]))
    assert o2.shape == (24,) and np.isfinite(o2).all() and np.isfinite(r)
    # the doors that stay shut
    with pytest.raises(ValueError):
        E.make("BipedalWalkerHardcore-v2", model="walker", **kw)                       # the name without the word
    with pytest.raises(ValueError, match="do not agree"):
        E.make("BipedalWalker-v2", model="walker", terrain="hardcore", **kw)           # name and terrain mismatch
    with pytest.raises(ValueError):
        E.make("BipedalWalkerHardcore-v2", terrain="hardcore", **kw)                   # no model
    with pytest.raises(ValueError, match="evaluation kernel"):
        E.make("BipedalWalkerHardcore-v2", model="walker", terrain="hardcore", on_device=True)
    with pytest.raises(ValueError, match="evaluation kernel"):
        E.make_device("BipedalWalkerHardcore-v2", model="walker", terrain="hardcore")
    g = E.make("BipedalWalker-v2", model="walker", terrain="grass", **kw)              # the grass word is accepted with the grass name
    assert g._vec.state_fields == NFW
