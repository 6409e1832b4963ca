"""GPU parity: HIP SAC1 learner / actor (through the C-ABI) vs the torch-CPU oracle on identical
weights, batch and explicit noise.

Tolerances (floating point; north star: losses within 1e-5 relative):
  * losses vs the float64 oracle: 1e-5 relative (observed ~1e-7..1e-6);
  * losses vs the float32 oracle: 1e-5 relative + the float32 oracle's own deviation from float64
    (the reference's literal (pi-mu)/(std+EPS) cancels catastrophically in float32 — see DESIGN.md
    §numerics and tests/test_oracle_sac1.py);
  * per-row q1/q2: 1e-5 abs+rel; logp_pi: vs float64 oracle 2e-5 relative;
  * gradients / parameters after the update: 2e-4 of the tensor's max |value| for gradients (float32
    accumulation over 256 rows), and parameter deltas within 1e-3 relative of the step size.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import sac1_oracle as so  # noqa: E402


@pytest.fixture(scope="module")
def ddrl():
    import distributed_drl_amd as d
    d._lib.require_gpu()
    return d


def _mk(ddrl, seed=0, **kw):
    from distributed_drl_amd.agent import HyperParameters, Learner
    opt = HyperParameters()
    for k, v in kw.items():
        setattr(opt, k, v)
    opt.seed = seed
    learner = Learner(opt)
    cfg = so.Config(obs_dim=opt.obs_dim, act_dim=opt.act_dim, hidden1=opt.hidden_sizes[0], hidden2=opt.hidden_sizes[1],
                    batch=opt.batch_size, alpha=opt.alpha, gamma=opt.gamma, lr=opt.lr, polyak=opt.polyak)
    return opt, learner, cfg


def _sp():
    """tests/_state_parity.py: start_from_other_targets / assert_targets_seen.  After set_weights the targets equal main and one update
    moves a target by (1 - polyak) lr at most — a quarter of the n * 2e-2 * lr bars below, which then pass whatever the polyak step
    does.  The tests that hold SAC1_TARGET to such a bar start from main != target instead (learner and oracle alike) and check that
    the bar is at most a tenth of the targets' movement."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import _state_parity
    return _state_parity


def _rel(a, b):
    return abs(float(a) - float(b)) / max(abs(float(b)), 1e-30)


def test_weight_roundtrip_and_layout(ddrl):
    opt, learner, cfg = _mk(ddrl)
    keys, vals = learner.get_weights()
    assert keys == [n for n, _ in so.param_specs(cfg)]
    ref = so.init_params(cfg, 0)  # same glorot/zeros init stream as the agent
    for k, v in zip(keys, vals):
        np.testing.assert_array_equal(v, ref[k])
    # target_init at set_weights (actor_learner.py:125-127)
    from distributed_drl_amd import _lib
    np.testing.assert_array_equal(learner.export(_lib.SAC1_TARGET).cpu().numpy(), so.flatten(ref))
    # subset set_weights
    learner.set_weights(keys[:2], [np.full_like(vals[0], 0.5), np.full_like(vals[1], -0.25)])
    k2, v2 = learner.get_weights()
    assert (v2[0] == 0.5).all() and (v2[1] == -0.25).all()
    np.testing.assert_array_equal(v2[2], vals[2])


@pytest.mark.parametrize("seed", [0, 3])
def test_first_update_matches_oracle(ddrl, seed):
    from distributed_drl_amd import _lib
    opt, learner, cfg = _mk(ddrl, seed)
    params = so.init_params(cfg, seed)
    rs = np.random.RandomState(seed + 10)
    for k in params:  # non-zero biases exercise every term
        if k.endswith("bias"):
            params[k] = rs.uniform(-0.05, 0.05, params[k].shape).astype(np.float32)
    learner.set_weights(list(params.keys()), list(params.values()))
    batch, eps = so.synthetic_batch(cfg, seed=1234 + seed)
    o32, o64 = so.Sac1Oracle(cfg, params, torch.float32), so.Sac1Oracle(cfg, params, torch.float64)
    w32, w64 = o32.step(batch, *eps), o64.step(batch, *eps)
    losses, (q1, q2, lp) = learner.train(batch, eps=eps, return_outputs=True)
    got = losses.cpu().numpy()
    for i, k in enumerate(("pi_loss", "q1_loss", "q2_loss")):
        assert _rel(got[i], w64[k]) <= 1e-5, (k, got[i], float(w64[k]))
        own = abs(float(w32[k]) - float(w64[k]))
        assert abs(got[i] - float(w32[k])) <= 1e-5 * abs(float(w64[k])) + own, k
    np.testing.assert_allclose(q1.cpu().numpy(), w64["q1"].numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(q2.cpu().numpy(), w64["q2"].numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(lp.cpu().numpy(), w64["logp_pi"].numpy(), rtol=2e-5, atol=2e-5)
    # gradients (pre-update parameters)
    g = learner.export(_lib.SAC1_GRAD).cpu().numpy()
    g64 = o64.flat("grads")
    off = 0
    for name, shape in so.param_specs(cfg):
        n = int(np.prod(shape))
        a, b = g[off:off + n], g64[off:off + n]
        assert np.abs(a - b).max() <= 2e-4 * max(np.abs(b).max(), 1e-12), (name, np.abs(a - b).max(), np.abs(b).max())
        off += n
    # parameters, Adam moments and polyak targets after the update
    for which, name in ((_lib.SAC1_MAIN, "main"), (_lib.SAC1_TARGET, "target"), (_lib.SAC1_ADAM_M, "m"),
                        (_lib.SAC1_ADAM_V, "v")):
        a, b = learner.export(which).cpu().numpy(), o64.flat(name)
        scale = np.abs(b).max()
        assert np.abs(a - b).max() <= 2e-4 * scale + 1e-12, (name, np.abs(a - b).max(), scale)
    # the first Adam step moves every parameter with a non-zero gradient by ~lr: compare deltas
    d_gpu = learner.export(_lib.SAC1_MAIN).cpu().numpy() - so.flatten(params)
    d_ref = o64.flat("main") - so.flatten(params).astype(np.float64)
    assert np.abs(d_gpu - d_ref).max() <= 2e-2 * cfg.lr  # float32 param ulp (~3e-8) vs lr 5e-5
    assert learner.opt_steps() == (1, 1)


def test_twenty_updates_track_oracle(ddrl):
    """Sequential updates (Adam state, running beta powers, polyak) stay within the float32 band."""
    from distributed_drl_amd import _lib
    opt, learner, cfg = _mk(ddrl, 1)
    params = so.init_params(cfg, 1)
    learner.set_weights(list(params.keys()), list(params.values()))
    o64 = so.Sac1Oracle(cfg, params, torch.float64)
    for it in range(20):
        batch, eps = so.synthetic_batch(cfg, seed=77 + it)
        w = o64.step(batch, *eps)
        losses, _ = learner.train(batch, eps=eps, return_outputs=True)
        got = losses.cpu().numpy()
        for i, k in enumerate(("pi_loss", "q1_loss", "q2_loss")):
            assert _rel(got[i], w[k]) <= 2e-5, (it, k, got[i], float(w[k]))
    a, b = learner.export(_lib.SAC1_MAIN).cpu().numpy(), o64.flat("main")
    assert np.abs(a - b).max() <= 20 * 2e-2 * cfg.lr
    a, b = learner.export(_lib.SAC1_TARGET).cpu().numpy(), o64.flat("target")
    assert np.abs(a - b).max() <= 1e-6
    assert learner.opt_steps() == (20, 20)


def test_compute_then_apply_equals_step(ddrl):
    from distributed_drl_amd import _lib
    _, l1, cfg = _mk(ddrl, 2)
    _, l2, _ = _mk(ddrl, 2)
    batch, eps = so.synthetic_batch(cfg, seed=5)
    l1.train(batch, eps=eps)
    g = l2.compute_gradients(batch, eps=eps)
    l2.apply_gradients(g)  # export -> import round trip of the gradient, as the all-reduce path does
    for which in (_lib.SAC1_MAIN, _lib.SAC1_TARGET, _lib.SAC1_ADAM_M, _lib.SAC1_ADAM_V):
        assert torch.equal(l1.export(which), l2.export(which))


def test_update_is_deterministic(ddrl):
    from distributed_drl_amd import _lib
    _, l1, cfg = _mk(ddrl, 4)
    _, l2, _ = _mk(ddrl, 4)
    for it in range(3):
        batch, eps = so.synthetic_batch(cfg, seed=it)
        a, _ = l1.train(batch, eps=eps, return_outputs=True)
        b, _ = l2.train(batch, eps=eps, return_outputs=True)
        assert torch.equal(a, b)
    assert torch.equal(l1.export(_lib.SAC1_MAIN), l2.export(_lib.SAC1_MAIN))


def test_other_shapes(ddrl):
    """Ragged sizes: batch not a multiple of 32, hidden sizes not multiples of the tile, act_dim 3."""
    from distributed_drl_amd import _lib
    opt, learner, cfg = _mk(ddrl, 5, obs_dim=5, act_dim=3, hidden_sizes=(70, 45), batch_size=37)
    assert learner._lib.ddrl_sac1_is_fused(learner._h) == 0
    params = so.init_params(cfg, 5)
    learner.set_weights(list(params.keys()), list(params.values()))
    batch, eps = so.synthetic_batch(cfg, seed=9)
    o64 = so.Sac1Oracle(cfg, params, torch.float64)
    w = o64.step(batch, *eps)
    losses, (q1, q2, lp) = learner.train(batch, eps=eps, return_outputs=True)
    for i, k in enumerate(("pi_loss", "q1_loss", "q2_loss")):
        assert _rel(losses[i].item(), w[k]) <= 1e-5, k
    g, g64 = learner.export(_lib.SAC1_GRAD).cpu().numpy(), o64.flat("grads")
    assert np.abs(g - g64).max() <= 2e-4 * np.abs(g64).max()


def test_actor_matches_oracle(ddrl):
    from distributed_drl_amd.agent import Actor, HyperParameters
    opt = HyperParameters()
    opt.seed = 0
    actor = Actor(opt, max_rows=4096)
    cfg = so.Config()
    params = so.init_params(cfg, 0)
    pi = {k: v for k, v in params.items() if "/pi/" in k}
    keys, vals = actor.get_weights()
    assert keys == list(pi.keys())
    for k, v in zip(keys, vals):
        np.testing.assert_array_equal(v, pi[k])
    rs = np.random.RandomState(0)
    for n in (1, 37, 4096):
        obs = rs.randn(n, 8).astype(np.float32)
        eps = rs.randn(n, 2).astype(np.float32)
        want = so.actor_act(cfg, params, obs, eps, dtype=torch.float64)
        got = actor.get_actions(obs, eps=eps).cpu().numpy()
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=2e-6)
        want = so.actor_act(cfg, params, obs, None, deterministic=True, dtype=torch.float64)
        got = actor.get_actions(obs, deterministic=True).cpu().numpy()
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=2e-6)
    a1 = actor.get_action(obs[0], eps=eps[:1])
    assert a1.shape == (2,) and a1.dtype == np.float32
    np.testing.assert_array_equal(a1, actor.get_actions(obs[:1], eps=eps[:1]).cpu().numpy()[0])


@pytest.mark.parametrize("per_graph", [4, 3])
def test_graph_loop_equals_eager_sample_noise_train(ddrl, per_graph):
    """ddrl_loop_run (hipGraph: the fused step with the optimizer in the wgrad epilogues, the next batch's
    sampler riding in a forward launch into the alternate input set, noise generated from the device counter,
    double-buffered optimizer state — an odd number of updates per graph ends on a copy node) == the same
    updates issued one by one through the public surface with ddrl_normal_fill noise — bit for bit."""
    import ctypes
    from distributed_drl_amd import _lib
    from distributed_drl_amd.agent import HyperParameters, Learner
    from distributed_drl_amd.workers import TrainDevice
    lib = _lib.load()
    opt = HyperParameters()
    opt.seed, opt.batch_size, opt.push_freq = 3, 256, 7
    rs = np.random.RandomState(0)
    n = 5000
    data = [rs.randn(n, 8).astype(np.float32), rs.uniform(-1, 1, (n, 2)).astype(np.float32), rs.randn(n).astype(np.float32),
            rs.randn(n, 8).astype(np.float32), (rs.rand(n) < 0.05).astype(np.float32)]
    rbs = []
    for _ in range(2):
        rb = ddrl.ReplayBufferSAC1(8, 2, 8192, seed=11)
        rb.store_batch(*(torch.from_numpy(x).cuda() for x in data))
        rbs.append(rb)
    keys, vals = Learner(opt).get_weights()
    ps = ddrl.ParameterServer(keys, vals)
    td = TrainDevice(ps, rbs[0], opt, updates_per_graph=per_graph)
    v0 = ps.version
    n_upd = 23
    td.run(n_upd)          # eager updates and graph replays mixed (chunks of <= 7 between pushes); pushes after updates 7, 14, 21
    ref = Learner(opt)
    B, a = 256, 2
    pushed = None
    for u in range(n_upd):
        batch = rbs[1].sample_batch_device(B)
        e = torch.empty(3 * B * a, device="cuda")
        _lib.check(lib.ddrl_normal_fill(_lib.dptr(e), e.numel(), td.noise_seed, u * 3 * B * a, _lib.stream_ptr()))
        e = e.view(3, B, a)
        ref.train(batch, eps=(e[0], e[1], e[2]))
        if (u + 1) % 7 == 0:
            pushed = ref.get_weights_flat().clone()
    for which in (_lib.SAC1_MAIN, _lib.SAC1_TARGET, _lib.SAC1_ADAM_M, _lib.SAC1_ADAM_V):
        assert torch.equal(td.agent.export(which), ref.export(which)), which
    assert td.agent.opt_steps() == (n_upd, n_upd)
    assert rbs[0].get_counts() == rbs[1].get_counts()
    k0, p0 = rbs[0].mt_state()
    k1, p1 = rbs[1].mt_state()
    assert p0 == p1 and (k0 == k1).all()
    assert ps.version == v0 + 3 and torch.equal(ps.pull_flat(0, td.agent.n_params), pushed)


class _DsacArgs:
    """What example/dsac.py:185-216 hands to Model(args)."""

    def __init__(self, obs_dim=8, act_dim=2, hid=(400, 300), batch_size=100, seed=0):
        self.obs_dim, self.act_dim = obs_dim, act_dim
        self.ac_kwargs = dict(hidden_sizes=list(hid))
        self.gamma = 0.99,          # dsac.py:198 really sets a 1-tuple
        self.polyak, self.lr, self.alpha, self.batch_size, self.seed, self.max_ep_len = 0.995, 1e-3, 0.2, batch_size, seed, 1000


@pytest.mark.parametrize("hid,batch", [((400, 300), 100), ((300, 300), 100), ((64, 48), 37), ((50, 34), 20)])
def test_sacv_model_matches_oracle(ddrl, hid, batch):
    """N4: the SAC-v learner of example/model.py (policy + twin Q + V + target V, batch 100, lr 1e-3,
    alpha 0.2 as example/dsac.py sets them): losses within 1e-5 relative of the float64 oracle over
    the first update (5e-5 over the next four), gradients / parameters / targets within the float32 band,
    same variable order."""
    from distributed_drl_amd import _lib
    from distributed_drl_amd.agent import Model
    from oracle import sacv_oracle as sv
    args = _DsacArgs(hid=hid, batch_size=batch, seed=3)
    model = Model(args)
    # the direct-operand kernels whenever the hidden sizes allow (example/dsac.py's own 300 x 2 at batch 100 included);
    # (50, 34) stays on the generic kernels
    import os
    assert model._lib.ddrl_sac1_is_fused(model._h) == (1 if hid[0] % 4 == 0 and hid[1] % 4 == 0 and not os.environ.get("DDRL_SAC1_GENERIC") else 0)
    cfg = so.Config(obs_dim=8, act_dim=2, hidden1=hid[0], hidden2=hid[1], batch=batch, alpha=0.2, gamma=0.99, lr=1e-3, polyak=0.995)
    keys, vals = model.get_weights()
    assert keys == [n for n, _ in sv.param_specs(cfg)]
    params = sv.init_params(cfg, 3)
    for k, v in zip(keys, vals):
        np.testing.assert_array_equal(v, params[k])
    rs = np.random.RandomState(1)
    for k in params:
        if k.endswith("bias"):
            params[k] = rs.uniform(-0.05, 0.05, params[k].shape).astype(np.float32)
    model.set_weights(list(params.keys()), list(params.values()))
    o64 = sv.SacVOracle(cfg, params, torch.float64, stable=True)
    t0 = _sp().start_from_other_targets(model, [o64], params)
    for it in range(5):
        b, eps = so.synthetic_batch(cfg, seed=40 + it)
        w = o64.step(b, eps[0])
        losses, (q1, q2, lp) = model.train(b, eps=eps, return_outputs=True)
        got = losses.cpu().numpy()
        # identical parameters at update 0: the north star's 1e-5; afterwards the float32 and float64
        # trajectories drift apart (lr = 1e-3, 20x SAC1's): 5e-5
        tol = 1e-5 if it == 0 else 5e-5
        for i, k in enumerate(("pi_loss", "q1_loss", "q2_loss", "v_loss")):
            assert _rel(got[i], w[k]) <= tol, (it, k, got[i], float(w[k]))
        np.testing.assert_allclose(q1.cpu().numpy(), w["q1"].numpy(), rtol=5 * tol, atol=5 * tol)
        np.testing.assert_allclose(lp.cpu().numpy(), w["logp_pi"].numpy(), rtol=5 * tol, atol=5 * tol)
        if it == 0:
            g, g64 = model.export(_lib.SAC1_GRAD).cpu().numpy(), o64.flat("grads")
            assert np.abs(g - g64).max() <= 2e-4 * np.abs(g64).max()
    a, b64 = model.export(_lib.SAC1_MAIN).cpu().numpy(), o64.flat("main")
    assert np.abs(a - b64).max() <= 5 * 2e-2 * cfg.lr
    a, b64 = model.export(_lib.SAC1_TARGET).cpu().numpy(), o64.flat("target")
    assert np.abs(a - b64).max() <= 5 * 2e-2 * cfg.lr
    _sp().assert_targets_seen(o64, t0, 5 * 2e-2 * cfg.lr)
    assert model.opt_steps() == (5, 5)
    # get_action: the policy head of the same variables (deterministic = tanh(mu))
    obs = b["obs1"][0]
    mu = sv.policy(o64.main, "main", torch.as_tensor(obs[None].astype(np.float64)), torch.zeros(1, 2, dtype=torch.float64), cfg)[0]
    np.testing.assert_allclose(model.get_action(obs, True), mu.numpy()[0], rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("obs,acts,hid,batch", [(8, 4, (400, 300), 128), (11, 3, (50, 34), 37)])
def test_ddqn_learner_matches_oracle(ddrl, obs, acts, hid, batch):
    """N4: Double-DQN learner (algos/dqn/actor_learner.py:19-107): q_loss within 1e-5 relative of the float64
    oracle on the first update (5e-5 over the next three: lr 1e-3), q output, gradients, parameters, targets."""
    from distributed_drl_amd import _lib, dqn
    from oracle import dqn_oracle as do

    class Opt:
        obs_dim, act_dim, hidden_size, gamma, lr, polyak, batch_size, seed = obs, acts, list(hid), 0.99, 1e-3, 0.995, batch, 2
    learner = dqn.Learner(Opt, "learner")
    cfg = do.Config(obs_dim=obs, n_actions=acts, hidden1=hid[0], hidden2=hid[1], batch=batch)
    keys, vals = learner.get_weights()
    assert keys == [n for n, _ in do.param_specs(cfg)]
    params = do.init_params(cfg, 2)
    for k, v in zip(keys, vals):
        np.testing.assert_array_equal(v, params[k])
    rs = np.random.RandomState(3)
    for k in params:
        if k.endswith("bias"):
            params[k] = rs.uniform(-0.1, 0.1, params[k].shape).astype(np.float32)
    learner.set_weights(list(params.keys()), list(params.values()))
    o64 = do.DqnOracle(cfg, params, torch.float64)
    t0 = _sp().start_from_other_targets(learner, [o64], params)
    for it in range(4):
        b = do.synthetic_batch(cfg, 10 + it)
        w = o64.step(b)
        loss, q = learner.train(b, it, return_outputs=True)
        tol = 1e-5 if it == 0 else 5e-5
        assert _rel(loss.item(), w["q_loss"]) <= tol, (it, loss.item(), float(w["q_loss"]))
        np.testing.assert_allclose(q.cpu().numpy(), w["q"].numpy(), rtol=10 * tol, atol=10 * tol)
        if it == 0:
            g, g64 = learner.export(_lib.SAC1_GRAD).cpu().numpy(), o64.flat("grads")
            assert np.abs(g - g64).max() <= 2e-4 * np.abs(g64).max()
    for which, name in ((_lib.SAC1_MAIN, "main"), (_lib.SAC1_TARGET, "target")):
        assert np.abs(learner.export(which).cpu().numpy() - o64.flat(name)).max() <= 4 * 2e-2 * cfg.lr
    _sp().assert_targets_seen(o64, t0, 4 * 2e-2 * cfg.lr)
    # Actor.get_action: argmax of the same network (0.97 greedy)
    actor = dqn.Actor(Opt, "worker")
    actor.set_weights(*learner.get_weights())
    x = b["obs1"][:1]
    qv = do.q_net(o64.main, "main", torch.as_tensor(x.astype(np.float64)))[0].numpy()
    np.testing.assert_allclose(actor.q_values(x)[0].cpu().numpy(), qv, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("obs,acts,hid,batch", [(8, 4, (400, 300), 128), (6, 5, (40, 28), 50)])
def test_sqn_learner_matches_oracle(ddrl, obs, acts, hid, batch):
    """N4: soft-Q learner (algos/sqn/actor_learner.py:19-78): q_loss (= q1_loss + q2_loss) within 1e-5 relative of the
    float64 oracle on the first update (5e-5 over the next three), q1 output, gradients, parameters, targets."""
    from distributed_drl_amd import _lib, dqn
    from oracle import dqn_oracle as do

    class Opt:
        obs_dim, act_dim, hidden_size, gamma, lr, polyak, batch_size, seed, alpha = obs, acts, list(hid), 0.99, 1e-3, 0.995, batch, 2, 0.1
    learner = dqn.LearnerSQN(Opt, "learner")
    cfg = do.Config(obs_dim=obs, n_actions=acts, hidden1=hid[0], hidden2=hid[1], batch=batch)
    keys, vals = learner.get_weights()
    assert keys == [n for n, _ in do.sqn_param_specs(cfg)]
    params = do.sqn_init_params(cfg, 2)
    for k, v in zip(keys, vals):
        np.testing.assert_array_equal(v, params[k])
    rs = np.random.RandomState(3)
    for k in params:
        if k.endswith("bias"):
            params[k] = rs.uniform(-0.1, 0.1, params[k].shape).astype(np.float32)
    learner.set_weights(list(params.keys()), list(params.values()))
    o64 = do.SqnOracle(cfg, params, 0.1, torch.float64)
    t0 = _sp().start_from_other_targets(learner, [o64], params)
    for it in range(4):
        b = do.synthetic_batch(cfg, 20 + it)
        w = o64.step(b)
        loss, q = learner.train(b, it, return_outputs=True)
        tol = 1e-5 if it == 0 else 5e-5
        assert _rel(loss.item(), w["q_loss"]) <= tol, (it, loss.item(), float(w["q_loss"]))
        np.testing.assert_allclose(q.cpu().numpy(), w["q"].numpy(), rtol=10 * tol, atol=10 * tol)
        if it == 0:
            g, g64 = learner.export(_lib.SAC1_GRAD).cpu().numpy(), o64.flat("grads")
            assert np.abs(g - g64).max() <= 2e-4 * np.abs(g64).max()
    for which, name in ((_lib.SAC1_MAIN, "main"), (_lib.SAC1_TARGET, "target")):
        assert np.abs(learner.export(which).cpu().numpy() - o64.flat(name)).max() <= 4 * 2e-2 * cfg.lr
    _sp().assert_targets_seen(o64, t0, 4 * 2e-2 * cfg.lr)
    actor = dqn.ActorSQN(Opt, "worker")
    actor.set_weights(*learner.get_weights())
    assert 0 <= actor.get_action(b["obs1"][0]) < acts and 0 <= actor.get_action(b["obs1"][0], True) < acts


@pytest.mark.parametrize("obs,act,hid,batch", [(6, 1, (64, 96), 64), (9, 3, (128, 100), 96), (8, 4, (512, 512), 32), (3, 2, (36, 8), 32),
                                               (8, 2, (400, 300), 128), (8, 2, (400, 300), 100), (8, 2, (300, 300), 37), (5, 3, (64, 40), 1)])
def test_fused_envelope_shapes(ddrl, obs, act, hid, batch):
    """Shapes inside the fused path's envelope other than the headline one (1-4 action dims, K ranges that are not
    multiples of the 32-unit layer-1 blocks, 1 to 16 column tiles, one sub-chunk per wave, batches that are not a
    whole number of 32-row tiles — the padding rows must carry no loss and no gradient): first update vs the
    float64 oracle — losses 1e-5 relative, gradients, parameters — and the per-row outputs."""
    from distributed_drl_amd import _lib
    import os
    opt, learner, cfg = _mk(ddrl, 7, obs_dim=obs, act_dim=act, hidden_sizes=hid, batch_size=batch)
    assert learner._lib.ddrl_sac1_is_fused(learner._h) == (0 if os.environ.get("DDRL_SAC1_GENERIC") else 1)
    params = so.init_params(cfg, 7)
    rs = np.random.RandomState(11)
    for k in params:
        if k.endswith("bias"):
            params[k] = rs.uniform(-0.05, 0.05, params[k].shape).astype(np.float32)
    learner.set_weights(list(params.keys()), list(params.values()))
    o64 = so.Sac1Oracle(cfg, params, torch.float64)
    t0 = _sp().start_from_other_targets(learner, [o64], params)
    for it in range(2):
        b, eps = so.synthetic_batch(cfg, seed=90 + it)
        w = o64.step(b, *eps)
        losses, (q1, q2, lp) = learner.train(b, eps=eps, return_outputs=True)
        tol = 1e-5 if it == 0 else 3e-5
        for i, k in enumerate(("pi_loss", "q1_loss", "q2_loss")):
            assert _rel(losses[i].item(), w[k]) <= tol, (it, k, losses[i].item(), float(w[k]))
        np.testing.assert_allclose(q1.cpu().numpy(), w["q1"].numpy(), rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(q2.cpu().numpy(), w["q2"].numpy(), rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(lp.cpu().numpy(), w["logp_pi"].numpy(), rtol=1e-4, atol=2e-5)
        if it == 0:
            g, g64 = learner.export(_lib.SAC1_GRAD).cpu().numpy(), o64.flat("grads")
            assert np.abs(g - g64).max() <= 2e-4 * np.abs(g64).max()
    for which, name in ((_lib.SAC1_MAIN, "main"), (_lib.SAC1_TARGET, "target")):
        assert np.abs(learner.export(which).cpu().numpy() - o64.flat(name)).max() <= 2 * 2e-2 * cfg.lr
    _sp().assert_targets_seen(o64, t0, 2 * 2e-2 * cfg.lr)
    assert learner.opt_steps() == (2, 2)


@pytest.mark.parametrize("variant,obs,acts,hid,batch,misalign", [("ddqn", 1024, 4, (400, 300), 32, False), ("ddqn", 1028, 3, (72, 40), 50, False),
                                                                 ("sqn", 1040, 5, (100, 60), 130, False), ("ddqn", 2048, 2, (32, 32), 64, True)])
def test_wide_layer1_shapes(ddrl, variant, obs, acts, hid, batch, misalign):
    """Wide observations (obs_dim >= 1024) take layer 1 through csrc/wide_l1.h — split-K tiled forward + reduce, tiled wgrad with
    the bias row, the caller's observation rows read in place by LDS-DMA.  Shapes off the headline one: K not a multiple of the
    32-deep stage, a last column unit of 8 of 32 hidden units, batches that are not whole 32-row units / 128-row tiles (the wgrad's K),
    five evaluations and two networks (SQN), and observation pointers that are not 16-byte aligned (staged copy instead of in
    place).  Two updates vs the float64 oracle."""
    from distributed_drl_amd import _lib, dqn
    from oracle import dqn_oracle as do

    class Opt:
        obs_dim, act_dim, hidden_size, gamma, lr, polyak, batch_size, seed, alpha = obs, acts, list(hid), 0.99, 1e-3, 0.995, batch, 2, 0.1
    sqn = variant == "sqn"
    learner = (dqn.LearnerSQN if sqn else dqn.Learner)(Opt, "learner")
    cfg = do.Config(obs_dim=obs, n_actions=acts, hidden1=hid[0], hidden2=hid[1], batch=batch)
    params = (do.sqn_init_params if sqn else do.init_params)(cfg, 2)
    rs = np.random.RandomState(3)
    for k in params:
        if k.endswith("bias"):
            params[k] = rs.uniform(-0.1, 0.1, params[k].shape).astype(np.float32)
    learner.set_weights(list(params.keys()), list(params.values()))
    o64 = do.SqnOracle(cfg, params, 0.1, torch.float64) if sqn else do.DqnOracle(cfg, params, torch.float64)
    t0 = _sp().start_from_other_targets(learner, [o64], params)
    for it in range(2):
        b = do.synthetic_batch(cfg, 30 + it)
        w = o64.step(b)
        fed = dict(b)
        if misalign:
            for k in ("obs1", "obs2"):
                flat = torch.zeros(batch * obs + 1, dtype=torch.float32, device="cuda")
                flat[1:] = torch.from_numpy(b[k]).reshape(-1).cuda()
                fed[k] = flat[1:].view(batch, obs)
                assert fed[k].data_ptr() % 16 == 4
        loss, q = learner.train(fed, it, return_outputs=True)
        tol = 2e-5 if it == 0 else 1e-4
        assert _rel(loss.item(), w["q_loss"]) <= tol, (it, loss.item(), float(w["q_loss"]))
        np.testing.assert_allclose(q.cpu().numpy(), w["q"].numpy(), rtol=10 * tol, atol=10 * tol)
        if it == 0:
            g, g64 = learner.export(_lib.SAC1_GRAD).cpu().numpy(), o64.flat("grads")
            assert np.abs(g - g64).max() <= 3e-4 * np.abs(g64).max()
    for which, name in ((_lib.SAC1_MAIN, "main"), (_lib.SAC1_TARGET, "target")):
        assert np.abs(learner.export(which).cpu().numpy() - o64.flat(name)).max() <= 2 * 2e-2 * cfg.lr
    _sp().assert_targets_seen(o64, t0, 2 * 2e-2 * cfg.lr)
    # the q output for fewer rows than the batch goes through the staged image
    x = b["obs1"][:3]
    qn = (do.q_net(o64.main, "main", torch.as_tensor(x.astype(np.float64))) if not sqn else None)
    if qn is not None:
        np.testing.assert_allclose(learner.q_values(x).cpu().numpy(), qn.numpy(), rtol=1e-3, atol=1e-4)


def test_stream_k_timeout_poisons_the_learner_until_it_gets_fresh_parameters(ddrl, monkeypatch):
    """k_wide_sk's combine gives up after ~1 s without its partner's slab and raises a sticky host-mapped word: that update's layer-1
    gradient was wrong, and every later step built on it.  The learner must then refuse to step AND to hand its parameters out
    (get_weights / export: a push or a checkpoint of corrupted weights) until it is given fresh ones; afterwards it runs the
    tile-per-workgroup kernel.  DDRL_SK_POISON_AFTER=n makes the host raise the word behind the n-th step."""
    from distributed_drl_amd import _lib, dqn

    class Opt:
        obs_dim, act_dim, hidden_size, gamma, lr, polyak, batch_size, seed, alpha = 28224, 4, [400, 300], 0.99, 1e-3, 0.995, 512, 2, 0.1
    monkeypatch.setenv("DDRL_SK_POISON_AFTER", "2")
    learner = dqn.Learner(Opt, "learner")
    monkeypatch.delenv("DDRL_SK_POISON_AFTER")
    keys, vals = learner.get_weights()
    g = torch.Generator(device="cuda").manual_seed(0)
    b = {"obs1": torch.randint(0, 256, (512, Opt.obs_dim), device="cuda", generator=g).float(), "obs2": torch.randint(0, 256, (512, Opt.obs_dim), device="cuda", generator=g).float(),
         "acts": torch.randint(0, 4, (512,), device="cuda", generator=g).float(), "rews": torch.randn(512, device="cuda", generator=g), "done": torch.zeros(512, device="cuda")}
    learner.train(b, 0)
    learner.train(b, 1)                       # the word is raised behind this step's launches
    with pytest.raises(_lib.DdrlError, match="k_wide_sk"):
        learner.get_weights()                 # seen with the stream drained: nothing corrupted leaves the learner
    with pytest.raises(_lib.DdrlError, match="k_wide_sk"):
        learner.train(b, 2)                   # sticky: not a one-off report
    learner.set_weights(keys, vals)           # fresh parameters: usable again (tile-per-workgroup layer-1 gradient from here on)
    learner.train(b, 3)
    k2, v2 = learner.get_weights()
    assert k2 == keys and all(np.isfinite(v).all() for v in v2)


def test_ddqn_learner_at_the_config5_observation_width(ddrl):
    """BASELINE config 5's learner input: flat 84x84x4 = 28 224-wide observations (algos/dqn/train.py:43-52) through the
    Double-DQN learner — layer 1 is a K = 28 224 GEMM (csrc/wide_l1.h).  One update vs the float64 oracle; the
    tolerances are wider than at K = 8 because 28 224 float32 products are summed per pre-activation (~sqrt(K) * 6e-8)."""
    from distributed_drl_amd import _lib, dqn
    from oracle import dqn_oracle as do
    obs, acts, hid, batch = 84 * 84 * 4, 4, (400, 300), 32

    class Opt:
        obs_dim, act_dim, hidden_size, gamma, lr, polyak, batch_size, seed = obs, acts, list(hid), 0.99, 1e-3, 0.995, batch, 2
    learner = dqn.Learner(Opt, "learner")
    cfg = do.Config(obs_dim=obs, n_actions=acts, hidden1=hid[0], hidden2=hid[1], batch=batch)
    params = do.init_params(cfg, 2)
    keys, vals = learner.get_weights()
    for k, v in zip(keys, vals):
        np.testing.assert_array_equal(v, params[k])
    o64 = do.DqnOracle(cfg, params, torch.float64)
    b = do.synthetic_batch(cfg, 10)
    b["obs1"], b["obs2"] = b["obs1"] / 16.0, b["obs2"] / 16.0        # keep the K = 28 224 pre-activations O(1)
    w = o64.step(b)
    loss, q = learner.train(b, 0, return_outputs=True)
    assert _rel(loss.item(), w["q_loss"]) <= 1e-4, (loss.item(), float(w["q_loss"]))
    np.testing.assert_allclose(q.cpu().numpy(), w["q"].numpy(), rtol=1e-3, atol=1e-4)
    g, g64 = learner.export(_lib.SAC1_GRAD).cpu().numpy(), o64.flat("grads")
    assert np.abs(g - g64).max() <= 1e-3 * np.abs(g64).max()
    assert np.abs(learner.export(_lib.SAC1_MAIN).cpu().numpy() - o64.flat("main")).max() <= 2e-2 * cfg.lr


def test_two_thousand_updates_stay_with_the_float32_and_float64_oracles(ddrl):
    """Long-horizon agreement (the 20-update test and the determinism soaks cannot see a slow drift — a running beta^t
    product, a polyak image, a double-buffered operand one update stale): 2 000 sequential updates on one seeded batch stream with the
    float32 and the float64 oracle stepped beside the HIP learner (tests/_long_horizon.py; table of a run: profiles/r05_long_horizon.txt).
    Two float32 trajectories of relu networks separate chaotically from the float64 one (both reach 4e-2 of max |value| after 2 000
    updates), so the band is the float32 ORACLE's own separation, not a constant:
      * every window of 200 updates, every loss: median |relative deviation from float64| of HIP <= 2.5 x the float32 oracle's + 2e-6
        (observed: 0.6-1.3 x);
      * main / target / Adam m / Adam v at updates 100 .. 2000: rms deviation of HIP <= 2 x the float32 oracle's (observed 0.9-1.1 x),
        at updates 1 and 10 below the float32 oracle's own (the literal (pi - mu) / std of the reference cancels in float32);
      * no trend: the HIP / oracle ratio of those rms deviations at update 2000 is not above 1.5 x the ratio at update 100."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import _long_horizon as lh
    opt, learner, cfg = _mk(ddrl, 4)
    params = so.init_params(cfg, 4)
    rs = np.random.RandomState(14)
    for k in params:
        if k.endswith("bias"):
            params[k] = rs.uniform(-0.05, 0.05, params[k].shape).astype(np.float32)
    threads = torch.get_num_threads()
    torch.set_num_threads(min(8, threads))   # small matrices: a few threads are faster than a whole host
    try:
        res = lh.run(learner, cfg, params, 2000)
    finally:
        torch.set_num_threads(threads)
    lines = []
    lh.report(res, lines.append)
    text = "\n".join(lines)
    rh, r32 = np.abs(res["rel_hip"]), np.abs(res["rel_32"])
    for s in range(0, 2000, 200):
        for i, k in enumerate(lh.LOSSES):
            mh, m32 = np.median(rh[s:s + 200, i]), np.median(r32[s:s + 200, i])
            assert mh <= 2.5 * m32 + 2e-6, "updates %d-%d %s: HIP %.2e vs float32 oracle %.2e\n%s" % (s + 1, s + 200, k, mh, m32, text)
    rows = {r["update"]: r for r in res["table"]}
    for upd, row in rows.items():
        for name in ("main", "target", "m", "v"):
            rms_hip, rms_32 = row[name][2], row[name][3]
            if upd >= 100:
                assert rms_hip <= 2.0 * rms_32 + 1e-9, "update %d %s: rms deviation HIP %.2e vs float32 oracle %.2e\n%s" % (upd, name, rms_hip, rms_32, text)
            else:
                assert rms_hip <= rms_32 + 1e-9, "update %d %s: rms deviation HIP %.2e above the float32 oracle's %.2e\n%s" % (upd, name, rms_hip, rms_32, text)
    for name in ("main", "target", "m"):
        early, late = rows[100][name][2] / rows[100][name][3], rows[2000][name][2] / rows[2000][name][3]
        assert late <= 1.5 * max(early, 1.0), "%s: HIP / oracle deviation ratio grew from %.2f (update 100) to %.2f (update 2000)\n%s" % (name, early, late, text)
    assert learner.opt_steps() == (2000, 2000)


def test_launch_table_resplit_is_bit_identical_to_the_unsplit_tables(tmp_path):
    """Round 5 moved work between the update's launches (part of the q2(x, a) dgrad from launch "bq" to "mid", the Q-head wgrads from "mid"
    to "pi", a second copy of q2's dgrad image) to keep every launch under a multiple of 256 tiles.  Same arithmetic per tile: after 40
    graph-loop updates the parameters, targets and Adam moments must equal — bit for bit — those of the round-4 tables (DDRL_BQ_SPLIT=0,
    read when a learner is created: one process per setting)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = """
import sys, zlib
sys.path.insert(0, %r)
import numpy as np, torch
import distributed_drl_amd as d
from distributed_drl_amd import _lib
from distributed_drl_amd.agent import HyperParameters
from distributed_drl_amd.workers import TrainDevice
opt = HyperParameters(); opt.seed, opt.batch_size, opt.push_freq = 7, 256, 10 ** 9
rs = np.random.RandomState(0); n = 6000
rb = d.ReplayBufferSAC1(8, 2, 8192, seed=11)
rb.store_batch(*(torch.from_numpy(x).cuda() for x in (rs.randn(n, 8).astype(np.float32), rs.uniform(-1, 1, (n, 2)).astype(np.float32),
                 rs.randn(n).astype(np.float32), rs.randn(n, 8).astype(np.float32), (rs.rand(n) < 0.05).astype(np.float32))))
td = TrainDevice(None, rb, opt, updates_per_graph=8)
td.run(40)
torch.cuda.synchronize()
print("CRC", [zlib.crc32(td.agent.export(w).cpu().numpy().tobytes()) for w in (_lib.SAC1_MAIN, _lib.SAC1_TARGET, _lib.SAC1_ADAM_M, _lib.SAC1_ADAM_V)], td.agent.opt_steps())
""" % root
    out = {}
    for split in ("1", "0"):
        env = dict(os.environ, DDRL_BQ_SPLIT=split)
        p = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert p.returncode == 0, p.stderr.decode("utf-8", "replace")[-2000:]
        out[split] = [l for l in p.stdout.decode().splitlines() if l.startswith("CRC")][0]
    assert out["1"] == out["0"], out


@pytest.mark.parametrize("variant", ["sac1", "sacv"])
def test_host_batch_fast_path_equals_the_device_path(ddrl, variant):
    """train(replay_buffer.sample_batch()) with NumPy arrays (the reference's learner loop body, example/dsac.py:142-144) takes a path of
    its own since round 5 — one asynchronous copy out of alternating page-locked blocks straight into the learner's input set, noise
    generated in place, no staging launch.  Seven updates (the staging blocks are reused from the third on, with the host mutating its
    arrays right after every call) must leave parameters, targets and Adam moments bit-identical to the same updates fed as device tensors
    with the same noise stream positions."""
    from distributed_drl_amd import _lib
    from distributed_drl_amd.agent import HyperParameters, Learner, Model
    lib = _lib.load()
    if variant == "sac1":
        opt = HyperParameters()
        opt.seed, opt.batch_size = 5, 256
        a_, b_ = Learner(opt), Learner(opt)
        B, o, a = 256, 8, 2
    else:
        args = _DsacArgs(batch_size=100, seed=5)
        a_, b_ = Model(args), Model(args)
        B, o, a = 100, 8, 2
    rs = np.random.RandomState(3)
    ctr = 0
    for it in range(7):
        batch = dict(obs1=rs.randn(B, o).astype(np.float32), obs2=rs.randn(B, o).astype(np.float32), acts=rs.uniform(-1, 1, (B, a)).astype(np.float32),
                     rews=rs.randn(B).astype(np.float32), done=(rs.rand(B) < 0.1).astype(np.float32))
        dev = {k: torch.from_numpy(v.copy()).cuda() for k, v in batch.items()}
        a_.train(batch)                                   # NumPy arrays: the fast path
        for v in batch.values():
            v += 1.0                                      # the caller's arrays may change as soon as train() has returned
        e = torch.empty(3 * B * a, device="cuda")
        _lib.check(lib.ddrl_normal_fill(_lib.dptr(e), e.numel(), b_._noise_seed, ctr, _lib.stream_ptr()))
        ctr += 3 * B * a
        e = e.view(3, B, a)
        b_.train(dev, eps=(e[0], e[1], e[2]))
    assert a_._fast is not False and a_._noise_ctr == ctr
    for which in (_lib.SAC1_MAIN, _lib.SAC1_TARGET, _lib.SAC1_ADAM_M, _lib.SAC1_ADAM_V):
        assert torch.equal(a_.export(which), b_.export(which)), which
