"""FreeRunningLoop over the three worker families: the discrete (DQN / SQN) pair and the n-step pair beside the continuous one of
tests/test_gpu_driver.py::test_free_running_loop_two_streams_equal_the_one_stream_order, whose pattern this file follows.

REFERENCE  the same launches issued on ONE stream (`streams=(st, st)`) in the order [pull, K vector steps, n updates, commit] per
segment.  Every configuration runs three times — two streams, one stream, two streams again — and the three runs must agree bit for bit
in the learner's parameters, the commit ring's arrays, counters and sampler state, the envs' observations and the actor's weights.

Shared sizes: 64 envs, hidden (64, 32), batch 32, 5 vector steps beside 9 updates per segment, 7 segments, push_freq 6, seed 3, a commit
ring of 2000 rows pre-filled with 300 seeded rows (where every step stores, 300 + 7 * 5 * 64 = 2540 rows wrap it)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

N_ENV, K, N_UPD, SEGMENTS, CAP, PRE = 64, 5, 9, 7, 2000, 300
LN = 3


@pytest.fixture(scope="module")
def ddrl():
    import distributed_drl_amd as d
    d._lib.require_gpu()
    return d


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        x, y = a[k], b[k]
        if torch.is_tensor(x):
            assert torch.equal(x, y), "%s: %s differs" % (what, k)
        elif isinstance(x, np.ndarray):
            np.testing.assert_array_equal(x, y, err_msg="%s: %s" % (what, k))
        else:
            assert x == y, "%s: %s is %r against %r" % (what, k, x, y)


def _ring_state(rb):
    st = {"ring." + k: v.clone() for k, v in rb.rings().items()}
    st["counts"] = rb._counts()
    key, pos = rb.mt_state()
    st["mt_key"], st["mt_pos"] = key.copy(), pos
    return st


def _three_runs(run_it, what):
    a, b, c = run_it(False), run_it(True), run_it(False)
    _same(a, b, what + ": two streams against the one-stream order")
    _same(a, c, what + ": two streams, run to run")
    return a


# ---- the n-step pair -------------------------------------------------------------------------------------------------------------
def _nstep_opt(fused=True, articulated=False, num_envs=N_ENV, cap=CAP):
    from distributed_drl_amd.agent import HyperParameters
    opt = HyperParameters()
    opt.num_envs, opt.hidden_sizes, opt.batch_size, opt.push_freq, opt.seed, opt.start_steps = num_envs, (64, 32), 32, 6, 3, -1
    opt.Ln, opt.action_repeat, opt.max_ep_len = LN, 2, 24           # an env's episode ends after at most 12 vector steps
    opt.buffer_size, opt.num_buffers = cap, 1
    opt.fused_nstep_rollout = fused
    if articulated:
        opt.env_model, opt.env_velocity_iterations, opt.env_position_iterations = "articulated", 8, 3
        opt.fused_nstep_rollout_articulated = fused
    return opt


def _windows(n, seed):
    rs = np.random.RandomState(seed)
    f = lambda *s: torch.from_numpy(rs.randn(*s).astype(np.float32)).cuda()
    return f(n, LN + 1, 8), f(n, LN, 2), f(n, LN), torch.zeros(n, LN, device="cuda")


def _nstep_pair(ddrl, opt, learner=True, prefill=PRE):
    from distributed_drl_amd.agent import Learner
    rb = ddrl.ReplayBufferNStep(opt, seed=5)
    if prefill:
        rb.store_batch(*_windows(prefill, 1))
    ps = ddrl.ParameterServer(*Learner(opt).get_weights())
    roll = ddrl.RolloutDeviceNStep(ps, rb, opt)
    tr = ddrl.TrainDevice(ps, rb, opt, updates_per_graph=4) if learner else None
    return rb, ps, roll, tr


def _nstep_run(ddrl, one_stream, **kw):
    opt = _nstep_opt(**kw)
    rb, ps, roll, tr = _nstep_pair(ddrl, opt)
    roll.step(1)                                      # the filling phase's last step: _learning turns true on the host
    assert roll._learning and roll._fused is bool(kw.get("fused", True))
    steps0 = rb.get_counts()[1]
    st = torch.cuda.current_stream()
    loop = ddrl.FreeRunningLoop(roll, tr, opt, steps_per_segment=K, updates_per_segment=N_UPD, streams=(st, st) if one_stream else None)
    assert isinstance(loop.stage[0], ddrl.ReplayBufferNStep) and loop.stage[0].max_size == K * N_ENV and roll.auto_pull is False
    loop.run(SEGMENTS)
    loop.close()
    assert (loop.env_steps, loop.updates) == (SEGMENTS * K * N_ENV, SEGMENTS * N_UPD)
    assert roll.rbs == [rb] and roll.auto_pull is True and ps.version >= 10
    samples, steps, size = rb.get_counts()
    committed = steps - steps0                        # read once, after close(): run() never learns it
    assert samples == SEGMENTS * N_UPD
    # the masked path is exercised: every env restarts its window at least once in 35 steps, so some steps store no row for it
    assert 0 < committed < SEGMENTS * K * N_ENV, committed
    out = _ring_state(rb)
    out.update(learner=tr.agent.get_weights_flat().cpu().numpy(), obs=roll.env.obs.clone(), actor=roll.actor.get_weights_flat().cpu().numpy(),
               committed=committed)
    return out


def test_nstep_pair_two_streams_equal_the_one_stream_order_fused_and_unfused(ddrl):
    """The fused step's cursor commit and the unfused store_masked both leave the segment's window count in the staging ring's device
    state; append_from commits it.  Each path equals its own one-stream order and is reproducible, and the two paths equal each other."""
    fused = _three_runs(lambda one: _nstep_run(ddrl, one, fused=True), "n-step, fused step")
    unfused = _three_runs(lambda one: _nstep_run(ddrl, one, fused=False), "n-step, unfused sequence")
    _same(fused, unfused, "n-step: fused against unfused")


def test_nstep_staging_changes_nothing(ddrl):
    """No learner, a server nobody pushes to: worker X stores K = 5 steps straight into ring A; worker Y, on the same seeds, into a
    staging ring that append_from then commits into ring B."""
    opt = _nstep_opt(cap=500)
    (a, _, x, _), (b, _, y, _) = (_nstep_pair(ddrl, opt, learner=False, prefill=40) for _ in range(2))
    stage = y._free_staging(K * N_ENV)
    assert isinstance(stage, ddrl.ReplayBufferNStep) and (stage.max_size, stage.Ln, stage.widths) == (K * N_ENV, LN, b.widths)
    y._free_store_into(stage)
    x.step(K)
    y.step(K)
    b.append_from(stage)
    y._free_store_into(b)
    sa, sb = _ring_state(a), _ring_state(b)
    _same(sa, sb, "direct stores against staging + append_from")
    assert sa["counts"][1] > 40 and y.rbs == [b]
    assert torch.equal(x.env.obs, y.env.obs)


# ---- the discrete pair -----------------------------------------------------------------------------------------------------------
def _dqn_opt(variant, adopt, articulated=False):
    d = dict(obs_dim=8, act_dim=4, hidden_size=[64, 32], gamma=0.99, lr=1e-3, polyak=0.995, batch_size=32, seed=3, alpha=0.1,
             num_envs=N_ENV, max_ep_len=40, start_steps=-1, num_nodes=1, num_buffers=1, push_freq=6, buffer_size=CAP, variant=variant,
             adopt=adopt)
    if articulated:
        d.update(env_model="articulated", env_velocity_iterations=8, env_position_iterations=3, fused_discrete_rollout_articulated=True)
    return type("Opt", (), d)()


def _dqn_rows(n, seed):
    rs = np.random.RandomState(seed)
    f = lambda *s: rs.randn(*s).astype(np.float32)
    rows = (f(n, 8), rs.randint(0, 4, n).astype(np.float32), f(n), f(n, 8), np.zeros(n, np.float32))
    return tuple(torch.from_numpy(x).cuda() for x in rows)


def _dqn_pair(ddrl, opt, per_graph, ring_in_trainer=True):
    from distributed_drl_amd import dqn
    L = dqn.LearnerSQN if opt.variant == "sqn" else dqn.Learner
    ps = ddrl.ParameterServer(*L(opt).get_weights())
    rb = ddrl.ReplayBufferDQN(opt, 0, seed=5)
    rb.store_batch(*_dqn_rows(PRE, 1))
    other = rb if ring_in_trainer else ddrl.ReplayBufferDQN(opt, 1, seed=6)
    roll = ddrl.RolloutDeviceDQN(ps, rb, opt)
    tr = ddrl.TrainDeviceDQN([ps], [[other]], opt, make_agent=lambda o_: L(o_, job="learner"), rng=np.random.RandomState(0),
                             updates_per_graph=per_graph)
    return rb, ps, roll, tr


def _dqn_run(ddrl, one_stream, variant, per_graph, adopt, articulated=False):
    from distributed_drl_amd import _lib
    opt = _dqn_opt(variant, adopt, articulated)
    rb, ps, roll, tr = _dqn_pair(ddrl, opt, per_graph)
    st = torch.cuda.current_stream()
    loop = ddrl.FreeRunningLoop(roll, tr, opt, steps_per_segment=K, updates_per_segment=N_UPD, streams=(st, st) if one_stream else None)
    assert isinstance(loop.stage[0], ddrl.ReplayBufferDQN) and not loop.stage[0].compact_obs and roll.auto_pull is False
    loop.run(SEGMENTS)
    loop.close()
    assert (loop.env_steps, loop.updates) == (SEGMENTS * K * N_ENV, SEGMENTS * N_UPD)
    assert roll.rb is rb and roll.auto_pull is True and roll._fused is True
    assert rb.get_counts() == (SEGMENTS * N_UPD, PRE + SEGMENTS * K * N_ENV, CAP)
    if per_graph:
        assert tr.loop_info(rb)[:2] == (per_graph, 1)
    out = _ring_state(rb)
    for name, which in (("main", _lib.SAC1_MAIN), ("target", _lib.SAC1_TARGET), ("adam_m", _lib.SAC1_ADAM_M), ("adam_v", _lib.SAC1_ADAM_V)):
        out["learner." + name] = tr.agent.export(which)
    out["obs"] = roll.env.obs.clone()
    for k, v in zip(*roll.actor.get_weights()):
        out["actor." + k] = np.array(v)
    return out


@pytest.mark.parametrize("adopt", ["step", "episode"])
@pytest.mark.parametrize("per_graph", [0, 4])
@pytest.mark.parametrize("variant", ["ddqn", "sqn"])
def test_discrete_pair_two_streams_equal_the_one_stream_order(ddrl, variant, per_graph, adopt):
    _three_runs(lambda one: _dqn_run(ddrl, one, variant, per_graph, adopt), "%s, updates_per_graph %d, adopt %s" % (variant, per_graph, adopt))


# ---- the articulated lander --------------------------------------------------------------------------------------------------------
def test_articulated_lander_under_the_loop(ddrl):
    """opt.env_model = "articulated" at 8 / 3 iterations with the workers' own fused flags: nothing of the loop looks at the model."""
    _three_runs(lambda one: _nstep_run(ddrl, one, fused=True, articulated=True), "n-step, articulated")
    _three_runs(lambda one: _dqn_run(ddrl, one, "ddqn", 4, "episode", articulated=True), "ddqn, articulated")


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_pairs_the_loop_refuses_and_what_close_restores(ddrl):
    opt = _nstep_opt()
    rb, ps, roll, tr = _nstep_pair(ddrl, opt)
    assert roll._learning is False                    # no step yet: the worker has not looked at the ring's counters
    with pytest.raises(ValueError, match="_learning"):
        ddrl.FreeRunningLoop(roll, tr, opt, steps_per_segment=K, updates_per_segment=N_UPD)
    assert roll.rbs == [rb] and roll.auto_pull is True

    rb2 = ddrl.ReplayBufferNStep(opt, seed=6)
    roll2 = ddrl.RolloutDeviceNStep(ps, [rb, rb2], opt)
    roll2._learning = True
    with pytest.raises(ValueError, match="exactly one ring"):
        ddrl.FreeRunningLoop(roll2, tr, opt, steps_per_segment=K, updates_per_segment=N_UPD)

    dopt = _dqn_opt("ddqn", "step")
    drb, _, droll, dtr = _dqn_pair(ddrl, dopt, 0, ring_in_trainer=False)
    with pytest.raises(ValueError, match="node_buffer"):
        ddrl.FreeRunningLoop(droll, dtr, dopt, steps_per_segment=K, updates_per_segment=N_UPD)
    assert droll.rb is drb and droll.auto_pull is True

    drb, _, droll, dtr = _dqn_pair(ddrl, dopt, 0)
    with pytest.raises(ValueError, match="must fit the replay ring"):
        ddrl.FreeRunningLoop(droll, dtr, dopt, steps_per_segment=CAP // N_ENV + 1, updates_per_segment=N_UPD)
    assert droll.rb is drb and droll.auto_pull is True

    # close() puts back what the loop found, an auto_pull the caller had turned off included
    droll.auto_pull = False
    loop = ddrl.FreeRunningLoop(droll, dtr, dopt, steps_per_segment=K, updates_per_segment=N_UPD)
    loop.run(1)
    assert droll.rb is loop.stage[0]
    loop.close()
    assert droll.rb is drb and droll.auto_pull is False
