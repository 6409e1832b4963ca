"""GPU: the SAC1 learner on n-step window rings (algos/sac1/sac_ray.py:40-51, 155-175) — the fold kernels against the NumPy float32
restatement (bit-exact), the folded update against the float64 oracle (the bars of tests/test_gpu_sac1.py), the device loop on a window
ring against the transition ring (Ln = 1) and against its own eager form (Ln = 8), and worker_train_nstep end to end.

The fold (include/ddrl.h, tests/_nstep_fold.py) is this project's definition of the n-step backup: the reference's learner does not
consume the windows its driver draws, so the float64 reference of every check here is that definition restated in NumPy.
tests/test_nstep_fold_cpu.py shows that the float32 fold's rounding moves the losses by < 2e-7 relative: under 2 % of the 1e-5 bar."""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _nstep_fold as nf  # noqa: E402
from oracle import sac1_oracle as so  # noqa: E402

NAMES = ("obs1", "obs2", "acts", "rews", "done")
WNAMES = ("obs", "acts", "rews", "done")


@pytest.fixture(scope="module")
def ddrl():
    import distributed_drl_amd as d
    d._lib.require_gpu()
    return d


def _opt(Ln=8, batch=256, obs_dim=8, act_dim=2, cap=256, num_buffers=1, seed=3, **kw):
    from distributed_drl_amd.agent import HyperParameters
    opt = HyperParameters(obs_dim=obs_dim, act_dim=act_dim)
    opt.Ln, opt.batch_size, opt.buffer_size, opt.num_buffers, opt.seed = Ln, batch, cap, num_buffers, seed
    for k, v in kw.items():
        setattr(opt, k, v)
    return opt


def _ring(ddrl, opt, win, seed=11):
    rb = ddrl.ReplayBufferNStep(opt, seed=seed)
    if win is not None:
        rb.store_batch(*(torch.from_numpy(win[k]).cuda() for k in WNAMES))
    return rb


def _same_bits(got, want, what):
    for k in NAMES:
        g = got[k].cpu().numpy() if torch.is_tensor(got[k]) else got[k]
        assert g.dtype == np.float32 and g.reshape(-1).tobytes() == np.ascontiguousarray(want[k]).reshape(-1).tobytes(), (what, k)


def _fold_on_device(win, Ln, obs_dim, act_dim, gamma, offset=0):
    """ddrl_nstep_fold through the C-ABI; offset: outputs start `offset` floats into their allocations (16-byte misalignment)."""
    from distributed_drl_amd import _lib
    lib = _lib.load()
    B = win["rews"].shape[0]
    src = [torch.from_numpy(np.ascontiguousarray(win[k])).cuda().reshape(B, -1) for k in WNAMES]
    out = {k: torch.empty(B * w + offset, dtype=torch.float32, device="cuda")[offset:] for k, w in zip(NAMES, (obs_dim, obs_dim, act_dim, 1, 1))}
    _lib.check(lib.ddrl_nstep_fold(*[_lib.dptr(t) for t in src], B, Ln, obs_dim, act_dim, gamma,
                                   *[ctypes.c_void_p(out[k].data_ptr()) for k in NAMES], _lib.stream_ptr()))
    return out


# ---- 1. ddrl_nstep_fold == the float32 restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("obs_dim", [8, 5])
@pytest.mark.parametrize("Ln", [1, 3, 8])
@pytest.mark.parametrize("B", [1, 37, 256])
def test_fold_kernel_is_bit_exact(ddrl, B, Ln, obs_dim):
    """obs_dim 8: the float4 path; 5: the scalar one.  Rows with the terminal at every position 0 .. Ln - 1, and with none (B == 1: one
    launch per position)."""
    rs = np.random.RandomState(1000 * obs_dim + 10 * Ln + B)
    gamma = 0.997
    for term in (range(Ln + 1) if B == 1 else ["every"]):
        win = nf.windows(rs, B, Ln, obs_dim, 2, terminal=term)
        _same_bits(_fold_on_device(win, Ln, obs_dim, 2, gamma), nf.fold32(win, gamma), (B, Ln, obs_dim, term))
    if Ln == 1:
        assert nf.fold32(win, gamma)["rews"].tobytes() == win["rews"][:, 0].tobytes()   # the identity the Ln = 1 ring test rests on


def test_fold_kernel_with_outputs_off_the_16_byte_grid(ddrl):
    rs = np.random.RandomState(5)
    win = nf.windows(rs, 37, 8, 8, 2, terminal="every")
    _same_bits(_fold_on_device(win, 8, 8, 2, 0.99, offset=1), nf.fold32(win, 0.99), "offset 1")


# ---- 2. draw + fold-gather in one launch == fold of the plain gather at the same indices ------------------------------------------
@pytest.mark.parametrize("stores,B,obs_dim,num_buffers", [(100, 256, 8, 1), (100, 37, 5, 2), (37, 37, 8, 1), (1, 37, 8, 2), (100, 5000, 8, 1),
                                                                  (100, 4096, 8, 1), (100, 4097, 8, 1), (100, 65537, 5, 1)])
def test_sample_nstep_device_equals_fold_of_the_gather(ddrl, stores, B, obs_dim, num_buffers):
    """Capacity 64: 100 stores wrap it, 37 fill it partly, 1 is the no-draw case of np.random.randint(0, 1, B); batch 5000 is beyond the
    one-workgroup sampler (index draw and fold-gather as two launches): 4096 is its last batch, 4097 the first of the wide draw, and
    65537 indices outgrow the handle's index scratch of 65536 in the gamma-0.5 draw, which passes no index buffer.  Same indices, MT19937
    state and counters as sample_batch_device."""
    Ln = 8
    opt = _opt(Ln=Ln, batch=B, obs_dim=obs_dim, cap=64, num_buffers=num_buffers)
    win = nf.windows(np.random.RandomState(stores + B), stores, Ln, obs_dim, 2, terminal="every")
    a, b = _ring(ddrl, opt, win), _ring(ddrl, opt, win)
    for it in range(2):
        got = a.sample_nstep_device(with_indices=True)
        plain = b.sample_batch_device(with_indices=True)
        assert torch.equal(got["idxs"], plain["idxs"])
        whole = b.gather_device(got["idxs"])
        for k in WNAMES:
            assert torch.equal(whole[k], plain[k]), k
        _same_bits(got, nf.fold32({k: whole[k].cpu().numpy() for k in WNAMES}, opt.gamma), (stores, B, it))
        ka, pa = a.mt_state()
        kb, pb = b.mt_state()
        assert pa == pb and (ka == kb).all()
        assert a.get_counts() == b.get_counts() == ((it + 1) * num_buffers, stores * num_buffers, min(stores, 64))
    other = a.sample_nstep_device(gamma=0.5)   # an explicit discount
    _same_bits(other, nf.fold32({k: v.cpu().numpy() for k, v in b.sample_batch_device().items()}, 0.5), "gamma 0.5")


def test_sample_nstep_device_refuses_what_it_cannot_do(ddrl):
    from distributed_drl_amd import _lib
    lib = _lib.load()
    with pytest.raises(ValueError, match="high <= 0"):
        _ring(ddrl, _opt(cap=64, batch=8), None).sample_nstep_device()
    rb = ddrl.ReplayBufferSAC1(8, 2, 64, seed=1)
    rb.store_batch(*(torch.zeros(4, w, device="cuda") for w in (8, 2, 1, 8, 1)))
    out = [torch.empty(8 * w, device="cuda") for w in (8, 8, 2, 1, 1)]
    rc = lib.ddrl_replay_sample_nstep(rb._h, 8, 0.99, *[_lib.dptr(t) for t in out], None, _lib.stream_ptr())
    assert rc == _lib.DDRL_ERR_UNSUPPORTED
    assert rb.get_counts() == (0, 4, 4)   # nothing was drawn


# ---- 3. Learner.train(window batch) against the float64 oracle on the float64-folded batch ------------------------------------------
@pytest.mark.parametrize("B", [37, 256])
def test_train_on_a_window_batch_matches_the_oracle(ddrl, B):
    from distributed_drl_amd import _lib
    from distributed_drl_amd.agent import Learner
    Ln, seed = 8, 2
    opt = _opt(Ln=Ln, batch=B, seed=seed)
    cfg = so.Config(obs_dim=opt.obs_dim, act_dim=opt.act_dim, hidden1=opt.hidden_sizes[0], hidden2=opt.hidden_sizes[1],
                    batch=B, alpha=opt.alpha, gamma=opt.gamma, lr=opt.lr, polyak=opt.polyak)
    params = so.init_params(cfg, seed)
    rs = np.random.RandomState(seed + 10)
    for k in params:  # non-zero biases exercise every term
        if k.endswith("bias"):
            params[k] = rs.uniform(-0.05, 0.05, params[k].shape).astype(np.float32)
    win = nf.windows(rs, B, Ln, opt.obs_dim, opt.act_dim, terminal="every")
    eps = [rs.randn(B, opt.act_dim).astype(np.float32) for _ in range(3)]
    o64 = so.Sac1Oracle(cfg, params, torch.float64)
    w64 = o64.step(nf.fold64(win, opt.gamma), *eps)

    def fresh():
        learner = Learner(opt)
        learner.set_weights(list(params.keys()), list(params.values()))
        return learner

    learner = fresh()
    losses, (q1, q2, lp) = learner.train(win, eps=eps, return_outputs=True)
    got = losses.cpu().numpy()
    for i, k in enumerate(("pi_loss", "q1_loss", "q2_loss")):
        rel = abs(float(got[i]) - float(w64[k])) / abs(float(w64[k]))
        print("B %d %s: %.9g oracle %.9g rel %.3g" % (B, k, got[i], float(w64[k]), rel))
        assert rel <= 1e-5, (k, got[i], float(w64[k]))
    np.testing.assert_allclose(q1.cpu().numpy(), w64["q1"].numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(q2.cpu().numpy(), w64["q2"].numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(lp.cpu().numpy(), w64["logp_pi"].numpy(), rtol=2e-5, atol=2e-5)
    g, g64 = learner.export(_lib.SAC1_GRAD).cpu().numpy(), o64.flat("grads")
    off = 0
    for name, shape in so.param_specs(cfg):
        n = int(np.prod(shape))
        a, b = g[off:off + n], g64[off:off + n]
        assert np.abs(a - b).max() <= 2e-4 * max(np.abs(b).max(), 1e-12), (name, np.abs(a - b).max(), np.abs(b).max())
        off += n
    for which, name in ((_lib.SAC1_MAIN, "main"), (_lib.SAC1_TARGET, "target"), (_lib.SAC1_ADAM_M, "m"), (_lib.SAC1_ADAM_V, "v")):
        a, b = learner.export(which).cpu().numpy(), o64.flat(name)
        assert np.abs(a - b).max() <= 2e-4 * np.abs(b).max() + 1e-12, (name, np.abs(a - b).max(), np.abs(b).max())
    assert learner.opt_steps() == (1, 1)
    # device-tensor windows: the same update, bit for bit
    dev = fresh()
    losses_d, _ = dev.train({k: torch.from_numpy(v).cuda() for k, v in win.items()}, eps=eps, return_outputs=True)
    assert torch.equal(losses_d, losses)
    for which in (_lib.SAC1_MAIN, _lib.SAC1_TARGET, _lib.SAC1_ADAM_M, _lib.SAC1_ADAM_V):
        assert torch.equal(dev.export(which), learner.export(which)), which
    # the n-step driver's call (sac_ray.py:171): train(batch, cnt) — cnt is not noise; the learner's own noise stream advances as ever.
    # train_device takes the windows the same way.
    with_cnt, without, folded = fresh(), fresh(), fresh()
    for cnt in (1, 2):
        with_cnt.train(win, cnt)
        without.train(win)
        folded.train(nf.fold32(win, opt.gamma))
    assert with_cnt._noise_ctr == without._noise_ctr == folded._noise_ctr == 2 * 3 * B * opt.act_dim
    for which in (_lib.SAC1_MAIN, _lib.SAC1_TARGET, _lib.SAC1_ADAM_M, _lib.SAC1_ADAM_V):
        assert torch.equal(with_cnt.export(which), without.export(which)), which
        assert torch.equal(with_cnt.export(which), folded.export(which)), which
    t1, t2 = fresh(), fresh()
    t1.train_device({k: torch.from_numpy(v).cuda() for k, v in win.items()})
    t2.train_device({k: torch.from_numpy(v).cuda() for k, v in nf.fold32(win, opt.gamma).items()})
    assert torch.equal(t1.export(_lib.SAC1_MAIN), t2.export(_lib.SAC1_MAIN)) and t1.opt_steps() == (1, 1)


def _state(agent):
    from distributed_drl_amd import _lib
    return [agent.export(w).clone() for w in (_lib.SAC1_MAIN, _lib.SAC1_TARGET, _lib.SAC1_ADAM_M, _lib.SAC1_ADAM_V)]


# ---- 4. Ln = 1: a window ring trains exactly like the transition ring -------------------------------------------------------------
@pytest.mark.parametrize("per_graph", [16, 2])
def test_one_step_window_ring_equals_the_transition_ring(ddrl, per_graph):
    """The same 64 transitions, the same seeds: five updates of the device loop (per_graph 16: all eager; 2: one eager update, then two
    replays of a captured pair with the fold-gather riding in the forward launch) leave bit-identical learners and samplers."""
    from distributed_drl_amd.workers import TrainDevice
    opt = _opt(Ln=1, batch=64, cap=64)
    win = nf.windows(np.random.RandomState(8), 64, 1, 8, 2, terminal="some")
    wr = _ring(ddrl, opt, win)
    tr = ddrl.ReplayBufferSAC1(8, 2, 64, seed=11)
    tr.store_batch(*(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in
                     (win["obs"][:, 0], win["acts"][:, 0], win["rews"][:, 0], win["obs"][:, 1], win["done"][:, 0])))
    tds = [TrainDevice(None, rb, opt, updates_per_graph=per_graph) for rb in (wr, tr)]
    for td in tds:
        td.run(5)
    torch.cuda.synchronize()
    for a, b in zip(_state(tds[0].agent), _state(tds[1].agent)):
        assert torch.equal(a, b)
    assert tds[0].agent.opt_steps() == tds[1].agent.opt_steps() == (5, 5)
    assert wr.get_counts() == tr.get_counts()
    (ka, pa), (kb, pb) = wr.mt_state(), tr.mt_state()
    assert pa == pb and (ka == kb).all()


# ---- 5. the captured loop on a window ring == the same updates issued eagerly -------------------------------------------------------
def test_graph_loop_on_a_window_ring_equals_eager(ddrl):
    """TrainDevice.run(6), two updates per graph (one eager update, two replays, one eager remainder) on an Ln = 8 ring of 200 windows ==
    six times sample_nstep_device -> train_device from the same seeds: parameters, optimizer state, MT19937 state and counters.
    (The transition-ring form of this is test_gpu_sac1.py::test_graph_loop_equals_eager_sample_noise_train.)"""
    from distributed_drl_amd.agent import Learner
    from distributed_drl_amd.workers import TrainDevice
    opt = _opt(Ln=8, batch=256, cap=256)
    win = nf.windows(np.random.RandomState(9), 200, 8, 8, 2, terminal="some")
    rbs = [_ring(ddrl, opt, win), _ring(ddrl, opt, win)]
    td = TrainDevice(None, rbs[0], opt, updates_per_graph=2)
    td.run(6)
    ref = Learner(opt, job="learner", index=0)
    ref._noise_seed = td.noise_seed
    for _ in range(6):
        ref.train_device(rbs[1].sample_nstep_device())
    torch.cuda.synchronize()
    for a, b in zip(_state(td.agent), _state(ref)):
        assert torch.equal(a, b)
    assert td.agent.opt_steps() == ref.opt_steps() == (6, 6)
    assert rbs[0].get_counts() == rbs[1].get_counts() == (6, 200, 200)
    (ka, pa), (kb, pb) = rbs[0].mt_state(), rbs[1].mt_state()
    assert pa == pb and (ka == kb).all()


# ---- 6. worker_train_nstep, default agent and cache -----------------------------------------------------------------------------
def test_worker_train_nstep_end_to_end(ddrl):
    """algos/sac1/sac_ray.py:155-175 with nothing faked: ParameterServer, ReplayBufferNStep (100 windows), the default Learner and
    BatchCache.  Three updates, weights left for the server after the third: they are those of three eager updates on the same draws
    (one buffer, one FIFO queue: the helper's first three draws are the learner's three batches)."""
    from distributed_drl_amd.agent import Learner
    opt = _opt(Ln=8, batch=64, cap=128)
    opt.max_updates = 3
    win = nf.windows(np.random.RandomState(10), 100, 8, 8, 2, terminal="some")
    rb, rb_ref = _ring(ddrl, opt, win), _ring(ddrl, opt, win)
    keys, vals = Learner(opt).get_weights()
    ps = ddrl.ParameterServer(keys, vals)
    assert ddrl.worker_train_nstep(ps, [rb], opt, 0, push_every=3) == 3
    ref = Learner(opt, job="learner")
    ref.set_weights(keys, vals)
    for _ in range(3):
        ref.train(rb_ref.sample_batch())
    pushed = ps.get_weights()
    rk, rv = ref.get_weights()
    assert list(pushed.keys()) == rk
    changed = False
    for k, v, v0 in zip(rk, rv, vals):
        np.testing.assert_array_equal(np.asarray(pushed[k]), v, err_msg=k)
        changed = changed or not np.array_equal(v, v0)
    assert changed
