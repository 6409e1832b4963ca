"""The fused rollout step on the ARTICULATED lander (ddrl_rollout_begin_articulated / ddrl_rollout_step_articulated, kernel
csrc/rollout3.hip) and RolloutDevice's opt-in to it (opt.fused_rollout_articulated): transitions and ring rows BIT-EXACT against
tests/lander3_oracle.py given the GPU's own actions, the actions against the float64 policy oracle and the unfused path, per-env
weight adoption against n reference workers, n_steps, the ring wrap, the refusals, and a run through ActorLearnerLoop.
Every test that uses a fused worker first asserts that the worker IS fused: a silent fallback to the unfused path fails."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

VIT, PIT = 8, 3   # the kernel's loops are run-time counts: the same code as at gym's 180 / 60 (test 2 runs those)
RINGS = ("obs1_buf", "obs2_buf", "acts_buf", "rews_buf", "done_buf")
EPLEN, EPI = 10, 13   # state rows of the per-env episode length / episode counter, on both models


@pytest.fixture(scope="module")
def ddrl():
    import distributed_drl_amd as d
    d._lib.require_gpu()
    return d


def _opt(n, max_ep_len, start_steps=-1, seed=11, vit=VIT, pit=PIT, flag=True, model="articulated"):
    from distributed_drl_amd.agent import HyperParameters
    opt = HyperParameters()
    opt.num_envs, opt.start_steps, opt.max_ep_len, opt.seed, opt.hidden_sizes = n, start_steps, max_ep_len, seed, (64, 48)
    if model != "simple":
        opt.env_model, opt.env_velocity_iterations, opt.env_position_iterations = model, vit, pit
    if flag is not None:
        opt.fused_rollout_articulated = flag
    return opt


def _oracle(opt):
    from lander3_oracle import Lander3Oracle
    return Lander3Oracle(opt.num_envs, seed=opt.seed, max_ep_len=opt.max_ep_len, velocity_iterations=opt.env_velocity_iterations,
                         position_iterations=opt.env_position_iterations)


def _weights(opt):
    from distributed_drl_amd.agent import Learner
    return Learner(opt).get_weights()


def _free_fall(keys, vals):
    """Engines off whatever the observation: zero kernels, mu = (-2, 0) -> a = (tanh(-2), 0), log_std at its floor."""
    out = []
    for k, w in zip(keys, vals):
        w = np.zeros_like(w)
        if "pi" in k and k.endswith("dense_2/bias"):
            w[0], w[1:] = -2.0, 0.0
        if "pi" in k and k.endswith("dense_3/bias"):
            w[:] = -40.0
        out.append(w)
    return out


def _coded_weights(keys, vals, v):
    """Policy version v as a recognisable action (tests/test_gpu_driver.py's): zero kernels, mu biases 0.08 (v % 40 + 1) and
    0.08 (v // 40 + 1), log_std at its floor."""
    out = []
    for k, w in zip(keys, vals):
        w = np.zeros_like(w)
        if "pi" in k and k.endswith("dense_2/bias"):
            w[0], w[1:] = 0.08 * (v % 40 + 1), 0.08 * (v // 40 + 1)
        if "pi" in k and k.endswith("dense_3/bias"):
            w[:] = -40.0
        out.append(w)
    return out


def _decode_version(acts):
    d = [np.rint(np.arctanh(np.clip(acts[:, c], -0.9999, 0.9999)) / 0.08 - 1).astype(int) for c in (0, 1)]
    assert np.allclose(acts[:, 0], np.tanh(0.08 * (d[0] + 1)), atol=1e-6) and np.allclose(acts[:, 1], np.tanh(0.08 * (d[1] + 1)), atol=1e-6)
    return d[0] + 40 * d[1]


def _worker(ddrl, opt, weights, capacity):
    from distributed_drl_amd.workers import RolloutDevice
    keys, vals = weights
    ps = ddrl.ParameterServer(keys, vals)
    rb = ddrl.ReplayBufferSAC1(8, 2, capacity, seed=0)
    return RolloutDevice(ps, rb, opt), rb, ps


def _lockstep(roll, rb, ora, steps, capacity, t0=0, fused_from=0):
    """`steps` vector steps of the worker beside the oracle, which is fed the worker's own actions: the next observation and the
    step's ring rows bit for bit after every step.  Returns the done and ended rows of the steps from `fused_from` on."""
    n = roll.env.n
    done, ended = [], []
    for t in range(t0, t0 + steps):
        obs = roll.env.obs.cpu().numpy().copy()
        np.testing.assert_array_equal(obs, ora.obs(), err_msg="obs before step %d" % t)
        roll.step()
        if t >= fused_from:
            assert roll._fused_live, "step %d did not take the fused launch" % t
        act = roll.act.cpu().numpy()
        o2, r, d, nxt, end = ora.step(act)
        np.testing.assert_array_equal(roll.env.obs.cpu().numpy(), nxt, err_msg="next obs, step %d" % t)
        rings = rb.rings()
        rows = (t * n + np.arange(n)) % capacity
        for k, w in zip(RINGS, (obs, o2, act, r, d)):
            got = rings[k].cpu().numpy()[rows].reshape(np.asarray(w).shape)
            np.testing.assert_array_equal(got, np.asarray(w, np.float32), err_msg="%s step %d" % (k, t))
        if t >= fused_from:
            done.append(np.asarray(d).copy())
            ended.append(np.asarray(end).copy())
    return np.array(done), np.array(ended)


def _check_end(roll, rb, ora, total_steps, capacity):
    n = roll.env.n
    np.testing.assert_array_equal(roll.env.get_state().cpu().numpy(), ora.S)
    ge, gr, gl = roll.env.stats()
    we, wr, wl = ora.stats()
    assert (ge, gl) == (we, wl)
    assert abs(gr - wr) <= 1e-9 * max(1.0, abs(wr))
    stored = total_steps * n
    assert rb.get_counts() == (0, stored, min(stored, capacity))
    assert rb.ptr == stored % capacity
    return ge


def test_transitions_and_ring_rows_bit_exact_given_the_gpus_actions(ddrl):
    """96 envs = two workgroups, the second half full, the cursor ticket crossing them; six unfused random steps first, so the
    fused path starts through the _fused_live refresh; then 100 fused steps of a free-fall policy: every env crashes."""
    n, fused_steps = 96, 100
    opt = _opt(n, 1000, start_steps=5)
    keys, vals = _weights(opt)
    cap = (6 + fused_steps) * n + 50
    roll, rb, _ = _worker(ddrl, opt, (keys, _free_fall(keys, vals)), cap)
    assert roll._fused_ready() is True and roll._versions
    ora = _oracle(opt)
    _lockstep(roll, rb, ora, 6, cap, fused_from=6)
    assert not roll._fused_live and roll.t == 6          # the random phase ran unfused
    done, _ = _lockstep(roll, rb, ora, fused_steps, cap, t0=6, fused_from=6)
    assert int((done == 1).sum()) >= n // 2                # not a degenerate run: terminal rows went through the fused store
    _check_end(roll, rb, ora, 6 + fused_steps, cap)


def test_the_same_at_gym_iterations_with_every_env_at_its_time_limit(ddrl):
    """180 / 60, 32 envs: half a wave, the idle lanes run the reductions and the tail; max_ep_len 6 inside 10 steps."""
    n, steps = 32, 10
    opt = _opt(n, 6, vit=180, pit=60)
    cap = steps * n + 7
    roll, rb, _ = _worker(ddrl, opt, _weights(opt), cap)
    assert roll._fused_ready() is True
    ora = _oracle(opt)
    done, ended = _lockstep(roll, rb, ora, steps, cap)
    assert ended[5].all() and not done[5].any()           # the time limit ends the episode and is not a terminal (dsac.py:109)
    assert ended.sum() == n
    assert _check_end(roll, rb, ora, steps, cap) == n


def test_actions_against_the_policy_oracle_and_the_unfused_path(ddrl):
    from distributed_drl_amd import _lib
    from oracle import sac1_oracle as so
    n, steps = 96, 4
    opt, opt_u = _opt(n, 40), _opt(n, 40, flag=None)
    keys, vals = _weights(opt)
    fused, rb, _ = _worker(ddrl, opt, (keys, vals), steps * n)
    plain, _, _ = _worker(ddrl, opt_u, (keys, vals), steps * n)
    assert fused._fused_ready() is True and plain._fused_ready() is False
    cfg = so.Config(hidden1=64, hidden2=48)
    params = dict(zip(keys, vals))
    for t in range(steps):
        obs = fused.env.obs.cpu().numpy().copy()
        ctr = fused.actor._noise_ctr
        fused.step()
        plain.step()
        act = rb.rings()["acts_buf"][t * n:(t + 1) * n].cpu().numpy()
        np.testing.assert_array_equal(act, fused.act.cpu().numpy())
        eps = torch.empty(n * 2, device="cuda")
        _lib.check(_lib.load().ddrl_normal_fill(_lib.dptr(eps), n * 2, fused.actor._noise_seed, ctr, _lib.stream_ptr()))
        want = so.actor_act(cfg, params, obs, eps.view(n, 2).cpu().numpy(), dtype=torch.float64)
        np.testing.assert_allclose(act, want, rtol=1e-5, atol=2e-6)
        # same policy, same eps stream: the two GPU paths differ only in the order of float32 sums
        np.testing.assert_allclose(act, plain.act.cpu().numpy(), rtol=0, atol=2e-6)
        plain.env.set_state(fused.env.get_state())   # keep the two env sets identical (their actions differ in the last bits)
        plain.env.obs.copy_(fused.env.obs)
    assert fused.actor._noise_ctr == plain.actor._noise_ctr == steps * n * 2


@pytest.mark.parametrize("n,limit,steps", [(64, 7, 40), (160, 23, 70)])
def test_each_env_acts_on_the_version_its_own_reference_worker_would_hold(ddrl, n, limit, steps):
    """tests/test_gpu_driver.py's test_vectorised_rollout_equals_n_reference_workers_in_the_weights_each_env_acts_on on the articulated
    model: bias-coded versions, staggered time limits, pushes between vector steps — a burst, one per step for longer than `limit`,
    a pause longer than `limit` (the single-version launch), then more."""
    opt = _opt(n, limit, seed=3)
    keys, vals = _weights(opt)
    roll, rb, ps = _worker(ddrl, opt, (keys, _coded_weights(keys, vals, 0)), n * steps)
    assert roll._fused_ready() is True
    assert roll._versions and roll.actor.n_slots == min(n, limit) + 2
    rs = np.random.RandomState(5)
    push_after, v = {}, 0
    for s in range(steps):
        if s < 6 or (10 <= s < 10 + limit + 3) or (s >= 10 + 2 * limit + 5 and rs.rand() < 0.5):
            k = 2 if s in (2, 3) else 1    # two pushes between two steps: only the later one is ever pulled
            v += k
            push_after[s] = (k, v)
    assert max(push_after) > 10 + 2 * limit + 5   # pushes resume after the pause
    eplen0 = np.arange(n) % limit
    st0 = roll.env.get_state()
    st0[EPLEN] = torch.from_numpy(eplen0).cuda().float()   # stagger the time limits: episode ends in every step, env by env
    roll.env.set_state(st0)
    epi_before = roll.env.get_state()[EPI].cpu().numpy().copy()
    assert (epi_before == 0).all()
    holds = np.zeros(n, int)                                  # the version env i's reference worker holds
    newest, max_live = 0, 0
    for s in range(steps):
        roll.step()
        assert roll._fused_live
        acts = rb.rings()["acts_buf"][s * n:(s + 1) * n].cpu().numpy()
        np.testing.assert_array_equal(_decode_version(acts), holds, err_msg="step %d" % s)
        state = roll.env.get_state().cpu().numpy()
        epi_after = state[EPI]
        if s == 0:   # rows 10 and 13 are the episode length and the episode counter on this model too (no crash in step 1)
            at_limit = eplen0 + 1 >= limit
            np.testing.assert_array_equal(state[EPLEN], np.where(at_limit, 0, eplen0 + 1))
            np.testing.assert_array_equal(epi_after, at_limit.astype(np.float32))
        holds[epi_after > epi_before] = newest               # episode ended in step s: reset, pull what the server holds
        epi_before = epi_after.copy()
        max_live = max(max_live, len(set(holds)))
        if s in push_after:
            k, newest = push_after[s]
            for j in range(k - 1, -1, -1):
                ps.push(keys, _coded_weights(keys, vals, newest - j))
    _, st = roll.actor.version_state()
    assert not st["out_of_slots"] and max_live >= min(limit, 6)
    assert roll.env.stats()[0] >= n * (steps // limit - 1)


def test_n_steps_in_one_call_equal_single_steps(ddrl):
    n, limit = 64, 5
    opt = _opt(n, limit)
    keys, vals = _weights(opt)
    _, vals1 = _weights(_opt(n, limit, seed=12))
    workers = [_worker(ddrl, opt, (keys, vals), 8 * n) for _ in range(2)]
    for roll, _, _ in workers:
        assert roll._fused_ready() is True and roll._versions
        st0 = roll.env.get_state()
        st0[EPLEN] = (torch.arange(n, device="cuda") % limit).float()   # two envs in five end their episode in every step
        roll.env.set_state(st0)
        roll.step()
        roll.step()
    for _, _, ps in workers:
        ps.push(keys, vals1)                                             # a second version goes live inside the steps compared
    (a, rba, _), (b, rbb, _) = workers
    a.step(4)
    for _ in range(4):
        b.step()
    assert a._fused_live and b._fused_live and a.t == b.t == 6
    assert a.actor._noise_ctr == b.actor._noise_ctr == 6 * n * 2
    ra, rbr = rba.rings(), rbb.rings()
    for k in RINGS:
        assert torch.equal(ra[k], rbr[k]), k
    assert rba.get_counts() == rbb.get_counts() == (0, 6 * n, 6 * n) and rba.ptr == rbb.ptr
    assert torch.equal(a.env.get_state(), b.env.get_state()) and torch.equal(a.env.obs, b.env.obs)
    assert torch.equal(a.act, b.act)
    (sa, sta), (sb, stb) = a.actor.version_state(), b.actor.version_state()
    assert torch.equal(sa, sb) and sta["newest"] == stb["newest"] and len(set(sa.cpu().numpy().tolist())) == 2
    assert a.env.stats() == b.env.stats()


@pytest.mark.parametrize("n,capacity", [(96, 200), (64, 40)])
def test_ring_wrap_and_rows_a_later_store_of_the_batch_overwrites(ddrl, n, capacity):
    """(96, 200): the cursor wraps inside the third step.  (64, 40): n > capacity, only the last 40 envs of a step are stored.
    The ring equals one filled by store_batch with the oracle's transitions in the same order."""
    opt = _opt(n, 40)
    roll, rb, _ = _worker(ddrl, opt, _weights(opt), capacity)
    assert roll._fused_ready() is True
    ref = ddrl.ReplayBufferSAC1(8, 2, capacity, seed=0)
    ora = _oracle(opt)
    for t in range(3):
        obs = ora.obs()
        np.testing.assert_array_equal(roll.env.obs.cpu().numpy(), obs)
        roll.step()
        assert roll._fused_live
        act = roll.act.cpu().numpy()
        o2, r, d, _, _ = ora.step(act)
        ref.store_batch(*(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda() for x in (obs, act, r, o2, d)))
    got, want = rb.rings(), ref.rings()
    for k in RINGS:
        assert torch.equal(got[k], want[k]), k
    assert rb.get_counts() == ref.get_counts() == (0, 3 * n, min(3 * n, capacity))
    assert rb.ptr == ref.ptr == (3 * n) % capacity


class _QOpt:
    obs_dim, act_dim, hidden_size, gamma, lr, polyak, batch_size, seed, alpha = 8, 4, [64, 48], 0.99, 1e-3, 0.995, 64, 3, 0.1
    num_envs, max_ep_len, start_steps, a_l_ratio, num_nodes, num_buffers, push_freq, buffer_size, variant = 32, 25, 0, 2, 1, 1, 50, 256, "ddqn"


def test_refusals_and_the_untouched_defaults(ddrl):
    from distributed_drl_amd import _lib
    from distributed_drl_amd.agent import Actor
    from distributed_drl_amd.env import VecLunarLander
    from distributed_drl_amd.replay import ReplayBufferDQN
    from distributed_drl_amd.workers import RolloutDevice
    lib = _lib.load()
    sp = _lib.stream_ptr()

    def ring(cls=None):
        rb = ReplayBufferDQN(_QOpt(), 0, seed=5) if cls else ddrl.ReplayBufferSAC1(8, 2, 256, seed=0)
        acts = torch.floor(torch.rand(40, device="cuda") * 4) if cls else torch.rand(40, 2, device="cuda")
        rb.store_batch(torch.rand(40, 8, device="cuda"), acts, torch.rand(40, device="cuda"), torch.rand(40, 8, device="cuda"),
                       torch.zeros(40, device="cuda"))   # some rows, so that "unchanged" is not "still empty"
        return rb

    def art(n):
        return VecLunarLander(n, seed=4, max_ep_len=50, model="articulated", velocity_iterations=VIT, position_iterations=PIT)

    cases = [("one-body", VecLunarLander(32, seed=4, max_ep_len=50), 32, ring(), True),
             ("n = 33", art(33), 33, ring(), True),
             ("1-D actions", art(32), 32, ring(ReplayBufferDQN), False)]
    for what, env, n, rb, begin_refused in cases:
        for _ in range(3):
            env.step(env.sample_actions())
        actor = Actor(_opt(n, 50), max_rows=n)
        probe = torch.rand(n, 8, device="cuda")

        def snapshot():
            torch.cuda.synchronize()
            snap = [env.get_state().clone(), env.obs.clone(), actor.get_actions(probe, deterministic=True).clone(),
                    torch.tensor(list(rb.get_counts()) + [rb.ptr])]
            return snap + [v.clone() for _, v in sorted(rb.rings().items())]

        calls = {"ddrl_rollout_step_articulated": lambda: lib.ddrl_rollout_step_articulated(env._h, actor._h, rb._h, 1, 1, 0, 0, None, None, sp)}
        if begin_refused:
            calls["ddrl_rollout_begin_articulated"] = lambda: lib.ddrl_rollout_begin_articulated(env._h, actor._h, sp)
        before = snapshot()
        for name, call in calls.items():
            assert call() == _lib.DDRL_ERR_UNSUPPORTED, (what, name)
            msg = lib.ddrl_last_error().decode()
            assert name in msg, (what, name, msg)
            if what == "one-body":   # ... and says which function takes this handle
                assert name.replace("_articulated", "") in msg.replace(name, ""), msg
            after = snapshot()
            assert len(after) == len(before)
            for k, (x, y) in enumerate(zip(before, after)):
                assert torch.equal(x, y), (what, name, k)
    # the defaults: the articulated worker stays unfused without the flag, the one-body worker is fused with or without it
    rb = ddrl.ReplayBufferSAC1(8, 2, 256, seed=0)
    for opt, want in ((_opt(32, 25, flag=None), False), (_opt(32, 25, flag=False), False),
                      (_opt(32, 25, flag=None, model="simple"), True), (_opt(32, 25, flag=True, model="simple"), True)):
        roll = RolloutDevice(ddrl.ParameterServer(*_weights(opt)), rb, opt)
        roll.step()
        assert roll._fused is want, (opt.__dict__, roll._fused)


def test_through_the_actor_learner_loop(ddrl):
    from distributed_drl_amd.workers import ActorLearnerLoop, RolloutDevice, TrainDevice
    n = 32
    opt = _opt(n, 25, start_steps=0, seed=2)
    opt.batch_size, opt.a_l_ratio, opt.push_freq = 32, 2, 8
    rb = ddrl.ReplayBufferSAC1(8, 2, 4096, seed=4)
    trainer = TrainDevice(None, rb, opt, updates_per_graph=4)
    keys, vals = trainer.agent.get_weights()
    ps = ddrl.ParameterServer(keys, vals)
    trainer.ps = ps
    roll = RolloutDevice(ps, rb, opt)
    assert roll._fused_ready() is True
    w0 = trainer.agent.get_weights_flat().clone()
    loop = ActorLearnerLoop(roll, trainer, opt)
    loop.run(4)
    torch.cuda.synchronize()
    assert roll._fused_live and roll.t == 4
    assert loop.counts()[:2] == (4 * n // 2, 4 * n)
    w1 = trainer.agent.get_weights_flat()
    assert torch.isfinite(w1).all() and not torch.equal(w0, w1)
