"""GPU: the early-requested prologue inputs of the SAC1 update's launches (sac1_direct.h).

k_dfwd<1> forms the addresses of the policy-head biases and of the noise rows from its preloaded scalars (the biases at
pi_bmu_off / pi_bls_off of the main or target copy, the noise items behind the inputs of the input set), and k_dg "bq" requests
rew / done / logp / b3 beside the head partials.  A wrong offset, parameter copy, noise item or input set reads a valid address
with the wrong value, so every case is held to the float64 oracle, with the bars tests/test_gpu_sac1.py uses at these shapes
(they are literals inside its test functions: test_fused_envelope_shapes itself is run at every shape here, and the Adam
moments take test_first_update_matches_oracle's 2e-4 of the tensor's max |value|).

Shapes: one row tile; padding rows (batch 37: clamped addresses must not leak into the losses); act_dim 1; act_dim 4 (the
d1 > 2 branch of the partial loads); hidden (32, 32); hidden (400, 300).  Each once with the device's own noise (generated
into the input set by k_dfwd<0>) and once with that same noise supplied by the caller: both against the oracle, and bit-equal
to each other.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import sac1_oracle as so  # noqa: E402
from test_gpu_sac1 import _DsacArgs, _mk, _rel, _sp, ddrl  # noqa: E402,F401
from test_gpu_sac1 import test_fused_envelope_shapes as _envelope_case  # noqa: E402
from test_gpu_sac1 import test_sacv_model_matches_oracle as _sacv_case  # noqa: E402

SHAPES = [(8, 2, (64, 64), 32), (8, 2, (64, 64), 37), (6, 1, (64, 96), 64), (8, 4, (64, 64), 64), (8, 2, (32, 32), 64), (8, 2, (400, 300), 64)]
STATE = ("SAC1_MAIN", "SAC1_TARGET", "SAC1_ADAM_M", "SAC1_ADAM_V")


def _biased_params(cfg, seed):
    params = so.init_params(cfg, seed)
    rs = np.random.RandomState(seed + 4)
    for k in params:   # non-zero biases: a head bias read from the wrong place must show
        if k.endswith("bias"):
            params[k] = rs.uniform(-0.05, 0.05, params[k].shape).astype(np.float32)
    return params


def _device_batch(b):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in b.items()}


def _device_noise(learner, cfg):
    """The three noise tensors the device generated into input set 0 (items 5..7)."""
    from distributed_drl_amd.replay import _view
    bufs = (ctypes.c_void_p * 8)()
    from distributed_drl_amd import _lib
    _lib.check(learner._lib.ddrl_sac1_input_buffers(learner._h, 0, bufs))
    dev = torch.device("cuda", torch.cuda.current_device())
    return [_view(bufs[i], (cfg.batch, cfg.act_dim), dev).clone() for i in (5, 6, 7)]


def _check_state(learner, o64, cfg, n_updates):
    """Bars of tests/test_gpu_sac1.py: parameters and targets as test_fused_envelope_shapes (n * 2e-2 * lr), Adam moments as
    test_first_update_matches_oracle (2e-4 of the tensor's max |value|)."""
    from distributed_drl_amd import _lib
    for which, name in ((_lib.SAC1_MAIN, "main"), (_lib.SAC1_TARGET, "target")):
        d = np.abs(learner.export(which).cpu().numpy() - o64.flat(name)).max()
        print(name, d, n_updates * 2e-2 * cfg.lr)
        assert d <= n_updates * 2e-2 * cfg.lr, (name, d)
    for which, name in ((_lib.SAC1_ADAM_M, "m"), (_lib.SAC1_ADAM_V, "v")):
        a, b = learner.export(which).cpu().numpy(), o64.flat(name)
        print(name, np.abs(a - b).max(), 2e-4 * np.abs(b).max())
        assert np.abs(a - b).max() <= 2e-4 * np.abs(b).max() + 1e-12, (name, np.abs(a - b).max(), np.abs(b).max())


def _check_outputs(losses, rows, w, tol):
    """test_fused_envelope_shapes' bars: losses `tol` relative, q1 / q2 rows 1e-4 + 1e-5, logp rows 1e-4 + 2e-5."""
    q1, q2, lp = rows
    for i, k in enumerate(("pi_loss", "q1_loss", "q2_loss")):
        print(k, losses[i].item(), float(w[k]))
        assert _rel(losses[i].item(), w[k]) <= tol, (k, losses[i].item(), float(w[k]))
    np.testing.assert_allclose(q1.cpu().numpy(), w["q1"].numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(q2.cpu().numpy(), w["q2"].numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(lp.cpu().numpy(), w["logp_pi"].numpy(), rtol=1e-4, atol=2e-5)


@pytest.mark.parametrize("obs,act,hid,batch", SHAPES)
def test_supplied_noise_matches_oracle_at_the_envelope_bars(ddrl, obs, act, hid, batch):  # noqa: F811
    """The caller's noise: tests/test_gpu_sac1.py's own first-two-updates check (losses, q1 / q2 / logp rows, gradients, main and
    target parameters), with its bars, at this file's shapes."""
    _envelope_case(ddrl, obs, act, hid, batch)


@pytest.mark.parametrize("obs,act,hid,batch", SHAPES)
def test_device_noise_equals_the_same_noise_supplied(ddrl, obs, act, hid, batch):  # noqa: F811
    from distributed_drl_amd import _lib
    kw = dict(obs_dim=obs, act_dim=act, hidden_sizes=hid, batch_size=batch)
    _, dev, cfg = _mk(ddrl, 7, **kw)
    _, sup, _ = _mk(ddrl, 7, **kw)
    assert dev._lib.ddrl_sac1_is_fused(dev._h) == (0 if os.environ.get("DDRL_SAC1_GENERIC") else 1)
    params = _biased_params(cfg, 7)
    for ln in (dev, sup):
        ln.set_weights(list(params.keys()), list(params.values()))
    o64 = so.Sac1Oracle(cfg, params, torch.float64)
    t0 = _sp().start_from_other_targets(dev, [o64], params)
    _sp().start_from_other_targets(sup, [], params)
    b, _ = so.synthetic_batch(cfg, seed=90)
    dev.train_device(_device_batch(b))
    eps = _device_noise(dev, cfg)
    assert all(float(e.abs().max()) > 0 for e in eps)
    losses, rows = sup.train(b, eps=eps, return_outputs=True)
    for name in STATE:
        assert torch.equal(dev.export(getattr(_lib, name)), sup.export(getattr(_lib, name))), name
    w = o64.step(b, *(e.cpu().numpy() for e in eps))
    _check_outputs(losses, rows, w, 1e-5)
    _check_state(dev, o64, cfg, 1)
    _sp().assert_targets_seen(o64, t0, 2e-2 * cfg.lr)
    assert dev.opt_steps() == (1, 1) and sup.opt_steps() == (1, 1)


def test_three_updates_through_the_graph_loop(ddrl):  # noqa: F811
    """Three updates in one captured graph: both input sets (the sampler of update u fills the set update u + 1 reads) and both
    optimizer-state copies; the same updates issued one by one with the same sampled batches and ddrl_normal_fill noise are the
    reference (bit-equal), and those are held to the float64 oracle."""
    from distributed_drl_amd import _lib
    from distributed_drl_amd.agent import HyperParameters, Learner
    from distributed_drl_amd.workers import TrainDevice
    lib = _lib.load()
    opt = HyperParameters()
    opt.seed, opt.batch_size, opt.push_freq, opt.hidden_sizes = 3, 64, 300, (64, 64)
    B, a, n = 64, 2, 600
    rs = np.random.RandomState(0)
    data = [rs.randn(n, 8).astype(np.float32), rs.uniform(-1, 1, (n, 2)).astype(np.float32), rs.randn(n).astype(np.float32),
            rs.randn(n, 8).astype(np.float32), (rs.rand(n) < 0.05).astype(np.float32)]
    rbs = []
    for _ in range(2):
        rb = ddrl.ReplayBufferSAC1(8, 2, 1024, seed=11)
        rb.store_batch(*(torch.from_numpy(x).cuda() for x in data))
        rbs.append(rb)
    td = TrainDevice(None, rbs[0], opt, updates_per_graph=3)
    td.run(3)
    ref = Learner(opt)
    cfg = so.Config(obs_dim=8, act_dim=2, hidden1=64, hidden2=64, batch=B, alpha=opt.alpha, gamma=opt.gamma, lr=opt.lr, polyak=opt.polyak)
    keys, vals = ref.get_weights()
    o64 = so.Sac1Oracle(cfg, dict(zip(keys, vals)), torch.float64)
    for u in range(3):
        batch = rbs[1].sample_batch_device(B)
        e = torch.empty(3 * B * a, device="cuda")
        _lib.check(lib.ddrl_normal_fill(_lib.dptr(e), e.numel(), td.noise_seed, u * 3 * B * a, _lib.stream_ptr()))
        e = e.view(3, B, a)
        losses, rows = ref.train(batch, eps=(e[0], e[1], e[2]), return_outputs=True)
        w = o64.step({k: v.cpu().numpy() for k, v in batch.items() if k in ("obs1", "obs2", "acts", "rews", "done")}, *(x.cpu().numpy() for x in e))
        _check_outputs(losses, rows, w, 1e-5 if u == 0 else 3e-5)
    for name in STATE:
        assert torch.equal(td.agent.export(getattr(_lib, name)), ref.export(getattr(_lib, name))), name
    _check_state(td.agent, o64, cfg, 3)
    assert td.agent.opt_steps() == (3, 3)


def test_sacv_at_batch_100_hidden_300(ddrl):  # noqa: F811
    """SAC-v (its own launch tables over the same kernels): tests/test_gpu_sac1.py's check against the SAC-v oracle, with its bars."""
    _sacv_case(ddrl, (300, 300), 100)
