"""GPU parity at the edges of the fused SAC1 backward tiles (k_dg): partial row / column tiles and the dQ/da path at act 1 and 4,
units whose relu is off for every row (the dgrad's mask test), and the captured loop against eager updates.

Every comparison is against oracle/sac1_oracle.py in float64 with the bars of tests/test_gpu_sac1.py, applied PER PARAMETER BLOCK
(so.param_specs): 2e-4 of the block's own max |value| (float32 accumulation over the batch) — one bar over the whole flat vector
would let an error in the small layer-1 action rows or the head blocks pass; losses 1e-5 relative.
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


def _mk(seed, obs, act, hid, batch):
    from distributed_drl_amd.agent import HyperParameters, Learner
    opt = HyperParameters()
    opt.obs_dim, opt.act_dim, opt.hidden_sizes, opt.batch_size, opt.seed = obs, act, hid, batch, seed
    learner = Learner(opt)
    assert learner._lib.ddrl_sac1_is_fused(learner._h) == 1
    cfg = so.Config(obs_dim=obs, act_dim=act, hidden1=hid[0], hidden2=hid[1], batch=batch, alpha=opt.alpha, gamma=opt.gamma,
                    lr=opt.lr, polyak=opt.polyak)
    return opt, learner, cfg


def _blocks(cfg, flat):
    off = 0
    for name, shape in so.param_specs(cfg):
        n = int(np.prod(shape))
        yield name, flat[off:off + n].reshape(shape)
        off += n
    assert off == flat.size


def _assert_blocks(cfg, got, want, what):
    for (name, a), (_, b) in zip(_blocks(cfg, got), _blocks(cfg, want)):
        err, bar = np.abs(a - b).max(), 2e-4 * np.abs(b).max() + 1e-12
        print("%s %s: max err %.3e, bar %.3e" % (what, name, err, bar))
        assert err <= bar, (what, name, err, bar)


def _rel(a, b):
    return abs(float(a) - float(b)) / max(abs(float(b)), 1e-30)


@pytest.mark.parametrize("obs,act,hid,batch", [(3, 1, (36, 40), 33), (8, 4, (40, 36), 31)])
def test_partial_tiles_match_oracle(ddrl, obs, act, hid, batch):
    """One and two row tiles with 31 / 1 padding rows, a partial last column tile in both dgrads, act 1 and 4 through the action rows
    of the dQ/da partials: gradients and losses after one update, parameters / targets / Adam moments after two."""
    from distributed_drl_amd import _lib
    opt, learner, cfg = _mk(7, obs, act, hid, batch)
    params = so.init_params(cfg, 7)
    rs = np.random.RandomState(17)
    for k in params:  # non-zero biases exercise every term
        if k.endswith("bias"):
            params[k] = rs.uniform(-0.05, 0.05, params[k].shape).astype(np.float32)
    learner.set_weights(list(params.keys()), list(params.values()))
    o64 = so.Sac1Oracle(cfg, params, torch.float64)
    for it in range(2):
        batch_, eps = so.synthetic_batch(cfg, seed=300 + it)
        w64 = o64.step(batch_, *eps)
        losses, _ = learner.train(batch_, eps=eps, return_outputs=True)
        got = losses.cpu().numpy()
        for i, k in enumerate(("pi_loss", "q1_loss", "q2_loss")):
            print("update %d %s: %.9g vs %.9g" % (it, k, got[i], float(w64[k])))
            assert _rel(got[i], w64[k]) <= 1e-5, (it, k, got[i], float(w64[k]))
        if it == 0:
            _assert_blocks(cfg, learner.export(_lib.SAC1_GRAD).cpu().numpy(), o64.flat("grads"), "grads")
    for which, name in ((_lib.SAC1_MAIN, "main"), (_lib.SAC1_TARGET, "target"), (_lib.SAC1_ADAM_M, "m"), (_lib.SAC1_ADAM_V, "v")):
        _assert_blocks(cfg, learner.export(which).cpu().numpy(), o64.flat(name), name)
    assert learner.opt_steps() == (2, 2)


def test_dead_units_get_exact_zero_gradients(ddrl):
    """Layer-1 units 0, 31, 32 and 67 of every network are off for every row (bias -1e3): their W1 column, b1 entry and W2 row get a
    gradient of exactly 0.0 — in the oracle first, then on the GPU — and every other unit gets a non-zero one.  The dgrad's mask
    compare must see the right element, with the right sense, at both ends of a column tile and in the partial last one."""
    from distributed_drl_amd import _lib
    dead = [0, 31, 32, 67]
    opt, learner, cfg = _mk(5, 8, 2, (68, 36), 64)
    params = so.init_params(cfg, 5)
    for net in ("pi", "q1", "q2"):
        params["main/%s/dense/bias" % net][dead] = -1e3
    learner.set_weights(list(params.keys()), list(params.values()))
    batch, eps = so.synthetic_batch(cfg, seed=41)
    o64 = so.Sac1Oracle(cfg, params, torch.float64)
    o64.step(batch, *eps)
    g64 = dict(_blocks(cfg, o64.flat("grads")))
    learner.train(batch, eps=eps)
    flat = learner.export(_lib.SAC1_GRAD).cpu().numpy()
    g = dict(_blocks(cfg, flat))
    live = [u for u in range(68) if u not in dead]
    for side, grads in (("oracle", g64), ("gpu", g)):   # the oracle first: the test cannot pass by both sides being wrong
        for net in ("pi", "q1", "q2"):
            w1, b1, w2 = grads["main/%s/dense/kernel" % net], grads["main/%s/dense/bias" % net], grads["main/%s/dense_1/kernel" % net]
            assert w1.shape[1] == 68 and b1.shape == (68,) and w2.shape == (68, 36)
            for u in dead:
                assert (w1[:, u] == 0.0).all() and b1[u] == 0.0 and (w2[u] == 0.0).all(), (side, net, u)
            for u in live:
                assert (w1[:, u] != 0.0).any() and b1[u] != 0.0 and (w2[u] != 0.0).any(), (side, net, u)
    _assert_blocks(cfg, flat, o64.flat("grads"), "grads")


def test_three_captured_updates_equal_three_eager_ones(ddrl):
    """(8, 2, (100, 68), 64): three updates replayed from the captured loop == the same three issued one by one — bit for bit on the
    parameters, the targets and both Adam moments."""
    from distributed_drl_amd import _lib
    from distributed_drl_amd.agent import HyperParameters, Learner
    from distributed_drl_amd.workers import TrainDevice
    lib = _lib.load()
    opt = HyperParameters()
    opt.seed, opt.batch_size, opt.hidden_sizes, opt.push_freq = 9, 64, (100, 68), 3
    rs = np.random.RandomState(2)
    n = 1000
    data = [rs.randn(n, 8).astype(np.float32), rs.uniform(-1, 1, (n, 2)).astype(np.float32), rs.randn(n).astype(np.float32),
            rs.randn(n, 8).astype(np.float32), (rs.rand(n) < 0.05).astype(np.float32)]
    rbs = []
    for _ in range(2):
        rb = ddrl.ReplayBufferSAC1(8, 2, 2048, seed=5)
        rb.store_batch(*(torch.from_numpy(x).cuda() for x in data))
        rbs.append(rb)
    keys, vals = Learner(opt).get_weights()
    ps = ddrl.ParameterServer(keys, vals)
    td = TrainDevice(ps, rbs[0], opt, updates_per_graph=3)
    assert lib.ddrl_sac1_is_fused(td.agent._h) == 1
    td.run(3)
    ref = Learner(opt)
    assert lib.ddrl_sac1_is_fused(ref._h) == 1
    B, a = 64, 2
    for u in range(3):
        batch = rbs[1].sample_batch_device(B)
        e = torch.empty(3 * B * a, device="cuda")
        _lib.check(lib.ddrl_normal_fill(_lib.dptr(e), e.numel(), td.noise_seed, u * 3 * B * a, _lib.stream_ptr()))
        e = e.view(3, B, a)
        ref.train(batch, eps=(e[0], e[1], e[2]))
    for which in (_lib.SAC1_MAIN, _lib.SAC1_TARGET, _lib.SAC1_ADAM_M, _lib.SAC1_ADAM_V):
        assert torch.equal(td.agent.export(which), ref.export(which)), which
    assert td.agent.opt_steps() == (3, 3)
