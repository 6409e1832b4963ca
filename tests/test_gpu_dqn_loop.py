"""ddrl_dqn_loop_* and TrainDeviceDQN(updates_per_graph > 0): the DQN / SQN learner's sample -> update loop on the device, replayed
from captured graphs.

REFERENCE  the eager path on a second learner and a second ring built from the same seeds: TrainDeviceDQN(updates_per_graph=0), i.e.
           ReplayBufferDQN.sample_batch_device + Learner.train per update — the path the float64 oracles and the reference-executed
           fixtures pin (tests/test_gpu_dqn.py, test_gpu_sqn.py, test_gpu_replay.py).  The loop runs the same draw on the same MT19937
           stream and the same launches on the same floats in the same order, so every comparison is torch.equal / ==: no tolerance.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

WALK = [1, 11, 7, 5, 16, 3, 1, 9]   # eager before the capture, the capturing call, full-size replays, every power-of-two remainder,
                                    # head / pre / tail variants, a length-1 tail
# launches ddrl_dqn_step issues eagerly on the narrow path (csrc/dqn.hip: dqn_step_launch): k_dqn_stage, layer-1 forward, layer-2
# forward, k_dqn_head, layer-2 backward, layer-1 wgrad, k_adam_polyak — each launch_gemm job list is ONE k_gemm launch (gemm_core.h)
S = 7
SHAPES = [(8, 4, [64, 48], 64),       # float4 gather, the lander's layout
          (6, 3, [20, 12], 37),       # scalar strided gather, a batch that is no multiple of a row tile or a head tile, an odd action count
          (8, 4, [400, 300], 128)]    # the lander's own learner


@pytest.fixture(scope="module")
def ddrl():
    import distributed_drl_amd as d
    d._lib.require_gpu()
    return d


def _opt(family, obs, act, hid, batch, cap, **kw):
    d = dict(obs_dim=obs, act_dim=act, hidden_size=list(hid), gamma=0.99, lr=1e-3, polyak=0.995, batch_size=batch, seed=3, alpha=0.1,
             num_nodes=1, num_buffers=1, push_freq=10 ** 9, buffer_size=cap, variant=family)
    d.update(kw)
    return type("Opt", (), d)()


def _agent(opt, family):
    """A learner that can also act (dqn.Actor / ActorSQN are Learner subclasses with get_actions), batch rows wide."""
    from distributed_drl_amd import dqn
    return (dqn.ActorSQN if family == "sqn" else dqn.Actor)(opt, "learner", max_rows=opt.batch_size)


def _rows(seed, n, obs, act, integer=False):
    rs = np.random.RandomState(seed)
    o = rs.randint(0, 256, (n, obs)).astype(np.float32) if integer else rs.randn(n, obs).astype(np.float32)
    o2 = rs.randint(0, 256, (n, obs)).astype(np.float32) if integer else rs.randn(n, obs).astype(np.float32)
    a = rs.randint(0, act, n).astype(np.float32)
    r = rs.randn(n).astype(np.float32)
    d = (rs.rand(n) < 0.2).astype(np.float32)
    return tuple(torch.from_numpy(x).cuda() for x in (o, a, r, o2, d))


def _trainer(opt, family, per_graph, n_rings=1, fill=None, ring_kw=None, rng_seed=0):
    """(trainer, rings): one learner, its parameter server, n_rings rings filled with `fill` seeded rows each."""
    from distributed_drl_amd.ps import ParameterServer
    from distributed_drl_amd.replay import ReplayBufferDQN
    from distributed_drl_amd.workers import TrainDeviceDQN
    seed_learner = _agent(opt, family)
    ps = ParameterServer(*seed_learner.get_weights())
    rings = [ReplayBufferDQN(opt, j, seed=5 + j, **(ring_kw or {})) for j in range(n_rings)]
    for j, rb in enumerate(rings):
        if fill:
            rb.store_batch(*_rows(100 + j, fill, opt.obs_dim, opt.act_dim, integer=bool((ring_kw or {}).get("compact_obs"))))
    t = TrainDeviceDQN([ps], [rings], opt, make_agent=lambda o_: _agent(o_, family), rng=np.random.RandomState(rng_seed),
                       updates_per_graph=per_graph)
    return t, rings


def _state(trainer, rings):
    from distributed_drl_amd import _lib
    st = {"loss": trainer.agent.loss.clone()}
    for name, which in (("main", _lib.SAC1_MAIN), ("target", _lib.SAC1_TARGET), ("adam_m", _lib.SAC1_ADAM_M), ("adam_v", _lib.SAC1_ADAM_V)):
        st[name] = trainer.agent.export(which)
    for j, rb in enumerate(rings):
        st["counts%d" % j] = rb.get_counts()        # (sample_times, steps, size)
        key, pos = rb.mt_state()
        st["mt_key%d" % j], st["mt_pos%d" % j] = key.copy(), pos
    return st


def _same(got, want, what):
    assert got.keys() == want.keys()
    for k in want:
        if torch.is_tensor(want[k]):
            assert torch.equal(got[k], want[k]), "%s: %s differs (max |diff| %.3e)" % (what, k, (got[k] - want[k]).abs().max().item())
        elif isinstance(want[k], np.ndarray):
            assert np.array_equal(got[k], want[k]), "%s: %s differs" % (what, k)
        else:
            assert got[k] == want[k], "%s: %s is %r, reference %r" % (what, k, got[k], want[k])


# ---- 1. bit-identity over a random walk ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_graph", [4, 5])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "o%d-a%d-h%dx%d-b%d" % (s[0], s[1], s[2][0], s[2][1], s[3]))
@pytest.mark.parametrize("family", ["ddqn", "sqn"])
def test_walk_is_bit_identical_to_the_eager_path(ddrl, family, shape, per_graph):
    obs, act, hid, batch = shape
    opt = _opt(family, obs, act, hid, batch, 4 * batch)          # 3 batch rows + the walk's 68: the stores wrap the two smaller rings
    got, g_rings = _trainer(opt, family, per_graph, fill=3 * batch)
    ref, r_rings = _trainer(opt, family, 0, fill=3 * batch)
    _same(_state(got, g_rings), _state(ref, r_rings), "before the walk")
    for i, k in enumerate(WALK):
        new = _rows(200 + i, 5 + i, obs, act)
        g_rings[0].store_batch(*new)
        r_rings[0].store_batch(*new)
        got.run(k)
        ref.run(k)
        _same(_state(got, g_rings), _state(ref, r_rings), "after run(%d), call %d" % (k, i))
    assert got.cnt == ref.cnt == 1 + sum(WALK)
    assert got.loop_info(g_rings[0])[:2] == (per_graph, 1)
    assert g_rings[0].get_counts()[0] == sum(WALK)
    # the acting forward repacks after a replay: q rows and greedy actions of a fixed observation batch
    x = torch.from_numpy(np.random.RandomState(9).randn(batch, obs).astype(np.float32)).cuda()
    assert torch.equal(got.agent.q_values(x), ref.agent.q_values(x))
    qa, qb = torch.empty(batch, act, device="cuda"), torch.empty(batch, act, device="cuda")
    a, b = got.agent.get_actions(x, q_out=qa, deterministic=True), ref.agent.get_actions(x, q_out=qb, deterministic=True)
    assert torch.equal(a, b) and torch.equal(qa, qb)
    assert not torch.equal(got.agent.export(), _agent(opt, family).export())     # (the walk did train)


# ---- 2. the captured update's shape -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_graph", [4, 5])
def test_captured_update_has_no_staging_launch(ddrl, per_graph):
    opt = _opt("ddqn", 8, 4, [64, 48], 64, 256)
    got, g_rings = _trainer(opt, "ddqn", per_graph, fill=192)
    ref, r_rings = _trainer(opt, "ddqn", 0, fill=192)
    got.run(per_graph - 1)
    assert got.loop_info(g_rings[0]) == (per_graph, 0, 0, 0)                    # shorter than a graph: eager, nothing captured yet
    got.run(per_graph)
    info = got.loop_info(g_rings[0])
    assert info[:2] == (per_graph, 1)
    assert info[2] == per_graph * (S - 1) + 1, info                             # the head sampler + S - 1 launches per update
    assert info[3] == 0 if per_graph % 2 == 0 else info[3] <= 1, info           # odd: at most the optimizer-state copy
    ref.run(2 * per_graph - 1)
    _same(_state(got, g_rings), _state(ref, r_rings), "after the capturing call")
    # a second call replays: nothing is captured again, and its updates are the reference's next ones, in order
    got.run(per_graph + 3)
    ref.run(per_graph + 3)
    assert got.loop_info(g_rings[0]) == info
    _same(_state(got, g_rings), _state(ref, r_rings), "after a replayed call")


def test_updates_per_graph_zero_is_always_eager_on_the_two_input_sets(ddrl):
    """The handle itself with updates_per_graph = 0 (TrainDeviceDQN never builds one: its 0 is the path without a handle)."""
    from distributed_drl_amd import _lib
    opt = _opt("sqn", 6, 3, [20, 12], 37, 148)
    got, g_rings = _trainer(opt, "sqn", 0, fill=111)
    ref, r_rings = _trainer(opt, "sqn", 0, fill=111)
    rc, h, _ = _create(got.agent, g_rings[0], per_graph=0)
    assert rc == 0 and h
    info = (ctypes.c_int32 * 4)()
    for k in (3, 1, 4):
        _lib.check(got.agent._lib.ddrl_dqn_loop_run(h, k, _lib.stream_ptr()))
        ref.run(k)
        _same(_state(got, g_rings), _state(ref, r_rings), "eager handle, run(%d)" % k)
        _lib.check(got.agent._lib.ddrl_dqn_loop_info(h, info))
        assert tuple(info) == (0, 0, 0, 0)
    _lib.check(got.agent._lib.ddrl_dqn_loop_destroy(h))


# ---- 3. refusals --------------------------------------------------------------------------------------------------------------------------
def _create(learner, rb, per_graph=4):
    from distributed_drl_amd import _lib
    h = ctypes.c_void_p()
    rc = learner._lib.ddrl_dqn_loop_create(ctypes.byref(h), learner._h, rb._h, per_graph, _lib.dptr(learner.loss))
    return rc, h, learner._lib.ddrl_last_error()


def test_refusals_leave_learner_and_ring_unchanged(ddrl):
    from distributed_drl_amd import _lib
    from distributed_drl_amd.replay import ReplayBufferDQN
    lib = _lib.load()
    # wide observations: the stream-K path stays out of graphs
    wide = _opt("ddqn", 1024, 3, [72, 40], 50, 200)
    tw, w_rings = _trainer(wide, "ddqn", 4, fill=150)
    before = _state(tw, w_rings)
    rc, h, msg = _create(tw.agent, w_rings[0])
    assert rc == _lib.DDRL_ERR_UNSUPPORTED and not h and b"wide" in msg
    _same(_state(tw, w_rings), before, "refused wide learner")
    # a compact (uint8) ring
    nar = _opt("ddqn", 8, 4, [64, 48], 64, 256)
    tc, c_rings = _trainer(nar, "ddqn", 4, fill=192, ring_kw=dict(compact_obs=True))
    before = _state(tc, c_rings)
    rc, h, msg = _create(tc.agent, c_rings[0])
    assert rc == _lib.DDRL_ERR_UNSUPPORTED and not h and b"compact" in msg
    _same(_state(tc, c_rings), before, "refused compact ring")
    # a ring of another observation width
    other = ReplayBufferDQN(_opt("ddqn", 6, 4, [64, 48], 64, 256), 0, seed=5)
    other.store_batch(*_rows(1, 100, 6, 4))
    c0, k0 = other.get_counts(), other.mt_state()
    rc, h, msg = _create(tc.agent, other)
    assert rc == _lib.DDRL_ERR_BAD_ARG and not h
    assert other.get_counts() == c0 and np.array_equal(other.mt_state()[0], k0[0]) and other.mt_state()[1] == k0[1]
    _same(_state(tc, c_rings), before, "refused ring width")
    # an empty ring: the eager first update reports it, nothing is captured
    te, e_rings = _trainer(nar, "ddqn", 4, fill=0)
    before = _state(te, e_rings)
    with pytest.raises(ValueError):
        te.run(6)
    assert te.loop_info(e_rings[0]) == (4, 0, 0, 0)
    lib.ddrl_last_error()
    _same(_state(te, e_rings), before, "empty ring")
    # a feed plan: refused at run
    tf, f_rings = _trainer(nar, "ddqn", 4, fill=192)
    plan = torch.full((8,), -1, dtype=torch.int32, device="cuda")
    f_rings[0].set_feed(plan, 64, [])
    before = _state(tf, f_rings)
    with pytest.raises(_lib.DdrlUnsupported):
        tf.run(6)
    _same(_state(tf, f_rings), before, "fed ring")
    f_rings[0].set_feed(None, 0, [])


@pytest.mark.parametrize("case", ["wide", "compact"])
def test_outside_the_envelope_the_trainer_falls_back(ddrl, case):
    opt = _opt("ddqn", 1024, 3, [72, 40], 50, 200) if case == "wide" else _opt("ddqn", 8, 4, [64, 48], 64, 256)
    kw = dict(compact_obs=True) if case == "compact" else None
    got, g_rings = _trainer(opt, "ddqn", 4, fill=150 if case == "wide" else 192, ring_kw=kw)
    ref, r_rings = _trainer(opt, "ddqn", 0, fill=150 if case == "wide" else 192, ring_kw=kw)
    got.run(1)
    ref.run(1)
    assert got.loop_info(g_rings[0]) is None and id(g_rings[0]) in got._loops     # decided once, remembered
    _same(_state(got, g_rings), _state(ref, r_rings), "fallback on a %s case" % case)
    got.run(5)
    ref.run(5)
    _same(_state(got, g_rings), _state(ref, r_rings), "fallback on a %s case, five more" % case)


# ---- 4. wiring ----------------------------------------------------------------------------------------------------------------------------
def _actor_learner_run(family, per_graph):
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
    trainer = TrainDeviceDQN([ps], [[rb]], opt, make_agent=lambda o_: L(o_, job="learner"), rng=np.random.RandomState(0),
                             updates_per_graph=per_graph)
    loop = ActorLearnerLoop(rollout, trainer, opt)
    rollout.auto_pull = False
    obs = torch.from_numpy(np.random.RandomState(13).randn(64, 8).astype(np.float32)).cuda()
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
    if per_graph:
        assert trainer.loop_info(rb)[:2] == (per_graph, 1)
    return _state(trainer, [rb]), dict(zip(keys, vals)), dict(zip(*rollout.actor.get_weights()))


@pytest.mark.parametrize("family", ["ddqn", "sqn"])
def test_rollout_device_dqn_under_the_actor_learner_loop_on_the_graph_path(ddrl, family):
    got, got_w, got_pushed = _actor_learner_run(family, 4)
    ref, ref_w, ref_pushed = _actor_learner_run(family, 0)
    _same(got, ref, "actor / learner loop, %s" % family)
    assert got_w.keys() == ref_w.keys()
    for k in ref_w:
        np.testing.assert_array_equal(got_w[k], ref_w[k], err_msg=k)
        np.testing.assert_array_equal(got_pushed[k], ref_pushed[k], err_msg="pushed " + k)     # a push saw the weights it sees eagerly


# ---- 5. two rings -------------------------------------------------------------------------------------------------------------------------
def test_two_rings_follow_the_host_draws(ddrl):
    opt = _opt("ddqn", 8, 4, [64, 48], 64, 256, num_buffers=2, push_freq=16)
    got, g_rings = _trainer(opt, "ddqn", 4, n_rings=2, fill=192, rng_seed=7)
    ref, r_rings = _trainer(opt, "ddqn", 0, n_rings=2, fill=192, rng_seed=7)
    assert got.run(40) == ref.run(40) == 40
    _same(_state(got, g_rings), _state(ref, r_rings), "two rings, run(40)")
    assert g_rings[0].get_counts()[0] + g_rings[1].get_counts()[0] == 40 and min(rb.get_counts()[0] for rb in g_rings) > 0
    a, b = got.rng.get_state(), ref.rng.get_state()
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]
    pushed = dict(zip(ref.keys, ref.node_ps[0].pull(ref.keys)))                  # the pushes behind updates 16 and 32
    for k, v in zip(got.keys, got.node_ps[0].pull(got.keys)):
        np.testing.assert_array_equal(v, pushed[k], err_msg="pushed " + k)
