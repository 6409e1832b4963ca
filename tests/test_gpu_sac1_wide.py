"""The wide SAC1 learner (ddrl_sac1_create_wide, include/ddrl_sac1_wide.h: k_dfwd_wide + k_dg over the mode-3 layer-1 blocks) against
the float64 / float32 oracles, with the cases, bars and helpers of tests/_state_parity.py and tests/test_gpu_learner_state.py (its
docstring states the bars): state per variable and over the whole vector at k = 2, every update's losses and rows.  Then the ways of
issuing an update on a wide handle (captured loop on a transition ring and on an n-step window ring == the eager sequence), and what
is refused: the envelope at create, the split API on a wide handle."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _nstep_fold as nf  # noqa: E402
import _state_parity as sp  # noqa: E402
import test_gpu_learner_state as ls  # noqa: E402
from _sac1_wide_cases import CASES, PATH_CASE  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ddrl():
    import distributed_drl_amd as d
    d._lib.require_gpu()
    return d


def _opt(case, **kw):
    from distributed_drl_amd.agent import HyperParameters
    opt = HyperParameters(obs_dim=case.obs, act_dim=case.act, act_scale=case.act_scale)
    opt.hidden_sizes, opt.batch_size, opt.seed = case.hid, case.batch, case.seed
    opt.alpha, opt.gamma, opt.lr, opt.polyak = case.alpha, case.gamma, case.lr, case.polyak
    opt.wide_learner = True
    for k, v in kw.items():
        setattr(opt, k, v)
    return opt


def _learner(case):
    from distributed_drl_amd.agent import Learner
    learner = Learner(_opt(case))
    assert learner._lib.ddrl_sac1_is_wide(learner._h) == 1 and learner._lib.ddrl_sac1_is_fused(learner._h) == 1, case.id
    return learner


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_wide_state_parity(ddrl, case):
    o64, w64, o32, w32 = sp.oracles(case)
    learner = _learner(case)
    _, _, _, batches = ls.load_start(case, learner)
    start = sp.start_of(case)
    np.testing.assert_array_equal(ls.exports(learner)["target"], start["target"])    # external -> mode 3 -> external; main != target from here on
    np.testing.assert_array_equal(ls.exports(learner)["main"], start["main"])
    grads = None
    for it, (b, eps) in enumerate(batches):
        got = ls.train(case, learner, b, eps, it)
        if it == 0:
            grads = learner.export(ls._codes()["grads"]).cpu().numpy()
        ls._check_outputs(case, it, got, w64[it], w32[it])
    ex = ls.exports(learner)
    ex["grads"] = grads
    rows = []
    try:
        sp.compare_state(ex, o64, o32, start, case.k, rows=rows)
    finally:
        print("\n".join(sp.format_rows(case.id, rows)))
    assert learner.opt_steps() == (case.updates, case.updates)


def test_wide_paths_equal_the_eager_sequence(ddrl):
    """27 / 4, hidden (72, 44), batch 37: six updates of the captured loop, three per graph, on a transition ring and on an n-step window
    ring (the folded windows into the input set a transition ring's draw fills) == train() on the same draws with the same noise."""
    from distributed_drl_amd.workers import TrainDevice
    case = PATH_CASE
    B, o, a, Ln = case.batch, case.obs, case.act, 8
    rs = np.random.RandomState(8)
    n = 200
    data = [rs.randn(n, o).astype(np.float32), rs.uniform(-1, 1, (n, a)).astype(np.float32), rs.randn(n).astype(np.float32),
            rs.randn(n, o).astype(np.float32), (rs.rand(n) < 0.05).astype(np.float32)]
    win = nf.windows(np.random.RandomState(9), n, Ln, o, a, terminal="some")
    opt = _opt(case, Ln=Ln, buffer_size=256, num_buffers=1)

    def transition_ring():
        rb = ddrl.ReplayBufferSAC1(o, a, 256, seed=11)
        rb.store_batch(*(torch.from_numpy(x).cuda() for x in data))
        return rb

    def window_ring():
        rb = ddrl.ReplayBufferNStep(opt, seed=11)
        rb.store_batch(*(torch.from_numpy(win[k]).cuda() for k in ("obs", "acts", "rews", "done")))
        return rb

    for make, draw in ((transition_ring, lambda rb: rb.sample_batch_device(B)), (window_ring, lambda rb: rb.sample_nstep_device())):
        rb_a, rb_b = make(), make()
        td = TrainDevice(None, rb_a, opt, updates_per_graph=3)
        assert td.agent._lib.ddrl_sac1_is_wide(td.agent._h) == 1
        ls.load_start(case, td.agent)
        ref = _learner(case)
        ls.load_start(case, ref)
        td.run(6)
        for u in range(6):
            ref.train(draw(rb_b), eps=ls._noise(ref, td.noise_seed, u, B, a))
        ls._assert_same(ls._state(td.agent), ls._state(ref), "captured loop on %s" % make.__name__)
        assert td.agent.opt_steps() == (6, 6) and rb_a.get_counts() == rb_b.get_counts()


@pytest.mark.parametrize("change", [dict(obs_dim=28, act_dim=4), dict(act_dim=5), dict(hidden1=402), dict(batch=513), dict(variant=1)],
                         ids=lambda c: "-".join("%s%d" % kv for kv in c.items()))
def test_wide_create_refuses(ddrl, change):
    from distributed_drl_amd import _lib
    from distributed_drl_amd.agent import HyperParameters
    lib = _lib.load()
    cfg = HyperParameters(obs_dim=24, act_dim=4).config(batch=256)
    for k, v in change.items():
        setattr(cfg, k, v)
    h = ctypes.c_void_p()
    with pytest.raises(_lib.DdrlUnsupported, match="ddrl_sac1_create_wide: "):
        _lib.check(lib.ddrl_sac1_create_wide(ctypes.byref(h), 0, ctypes.byref(cfg)))
    assert not h.value


def test_wide_handle_refuses_the_split_api(ddrl):
    from distributed_drl_amd import _lib
    case = PATH_CASE
    learner = _learner(case)
    cfg, _, _, batches = sp.make_setup(case)
    b, eps = batches[0]
    with pytest.raises(_lib.DdrlUnsupported, match="ddrl_sac1_compute_grads: "):
        learner.compute_gradients(b, eps=eps)
    with pytest.raises(_lib.DdrlUnsupported, match="ddrl_sac1_apply_grads: "):
        _lib.check(learner._lib.ddrl_sac1_apply_grads(learner._h, _lib.stream_ptr()))
    rb = ddrl.ReplayBufferSAC1(case.obs, case.act, 64, seed=1)    # (what dp_stepper's grads() calls between two batches)
    with pytest.raises(_lib.DdrlUnsupported, match="ddrl_sac1_compute_grads_and_sample: "):
        _lib.check(learner._lib.ddrl_sac1_compute_grads_and_sample(learner._h, 0, rb._h, 1, _lib.stream_ptr()))
