"""The wide SAC-v learner (agent.Model with wide_model: ddrl_sacv_create_wide, include/ddrl_sacv_wide.h — k_dfwd_wide + k_dg's SAC-v
jobs over the mode-3 layer-1 blocks of pi, q1, q2, V and target V) against the float64 / float32 SAC-v oracles, with the cases, bars and
helpers of tests/_state_parity.py and tests/test_gpu_learner_state.py (its docstring states the bars): state per variable and over the
whole vector at k = 2, every update's four losses and rows.  Then the captured loop on a transition ring and on an n-step window ring
== the eager sequence, and what is refused: the envelope at create, the split API on the handle."""
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
from _sacv_wide_cases import CASES, PATH_CASE  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ddrl():
    import distributed_drl_amd as d
    d._lib.require_gpu()
    return d


def _model(case):
    from distributed_drl_amd.agent import Model
    args = ls._Args(case)
    args.wide_model = True
    model = Model(args)
    assert model._lib.ddrl_sac1_is_wide(model._h) == 1 and model._lib.ddrl_sac1_is_fused(model._h) == 1, case.id
    return model


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_sacv_wide_state_parity(ddrl, case):
    o64, w64, o32, w32 = sp.oracles(case)
    model = _model(case)
    _, _, _, batches = ls.load_start(case, model)
    start = sp.start_of(case)
    np.testing.assert_array_equal(ls.exports(model)["target"], start["target"])    # external -> mode 3 -> external; main != target from here on
    np.testing.assert_array_equal(ls.exports(model)["main"], start["main"])
    grads = None
    for it, (b, eps) in enumerate(batches):
        got = ls.train(case, model, b, eps, it)
        if it == 0:
            grads = model.export(ls._codes()["grads"]).cpu().numpy()
        ls._check_outputs(case, it, got, w64[it], w32[it])
    ex = ls.exports(model)
    ex["grads"] = grads
    rows = []
    try:
        sp.compare_state(ex, o64, o32, start, case.k, rows=rows)
    finally:
        print("\n".join(sp.format_rows(case.id, rows)))
    assert model.opt_steps() == (case.updates, case.updates)


def test_sacv_wide_paths_equal_the_eager_sequence(ddrl):
    """27 / 4, hidden (72, 44), batch 37: six updates of the captured loop (ddrl_loop_* on the Model's handle: workers.TrainDevice builds
    a SAC1 Learner), three per graph, on a transition ring and on an n-step window ring == train() on the same draws with the same noise."""
    from distributed_drl_amd import _lib
    from distributed_drl_amd.agent import HyperParameters
    case = PATH_CASE
    B, o, a, Ln, seed = case.batch, case.obs, case.act, 8, 77
    rs = np.random.RandomState(8)
    n = 200
    data = [rs.randn(n, o).astype(np.float32), rs.uniform(-1, 1, (n, a)).astype(np.float32), rs.randn(n).astype(np.float32),
            rs.randn(n, o).astype(np.float32), (rs.rand(n) < 0.05).astype(np.float32)]
    win = nf.windows(np.random.RandomState(9), n, Ln, o, a, terminal="some")
    ring_opt = HyperParameters(obs_dim=o, act_dim=a)
    ring_opt.Ln, ring_opt.buffer_size, ring_opt.num_buffers = Ln, 256, 1

    def transition_ring():
        rb = ddrl.ReplayBufferSAC1(o, a, 256, seed=11)
        rb.store_batch(*(torch.from_numpy(x).cuda() for x in data))
        return rb

    def window_ring():
        rb = ddrl.ReplayBufferNStep(ring_opt, seed=11)
        rb.store_batch(*(torch.from_numpy(win[k]).cuda() for k in ("obs", "acts", "rews", "done")))
        return rb

    lib = _lib.load()
    for make, draw in ((transition_ring, lambda rb: rb.sample_batch_device(B)), (window_ring, lambda rb: rb.sample_nstep_device(B, case.gamma))):
        rb_a, rb_b = make(), make()
        looped, ref = _model(case), _model(case)
        ls.load_start(case, looped)
        ls.load_start(case, ref)
        loop = ctypes.c_void_p()
        _lib.check(lib.ddrl_loop_create(ctypes.byref(loop), looped._h, rb_a._h, 3, seed))
        try:
            _lib.check(lib.ddrl_loop_run(loop, 6, _lib.stream_ptr()))
            for u in range(6):
                ref.train(draw(rb_b), eps=ls._noise(ref, seed, u, B, a))
            ls._assert_same(ls._state(looped), ls._state(ref), "captured loop on %s" % make.__name__)
        finally:
            lib.ddrl_loop_destroy(loop)
        assert looped.opt_steps() == (6, 6) and rb_a.get_counts() == rb_b.get_counts()


@pytest.mark.parametrize("change", [dict(variant=0), dict(obs_dim=28, act_dim=4), dict(act_dim=5), dict(hidden1=402), dict(batch=513)],
                         ids=lambda c: "-".join("%s%d" % kv for kv in c.items()))
def test_sacv_wide_create_refuses(ddrl, change):
    from distributed_drl_amd import _lib
    from distributed_drl_amd.agent import HyperParameters
    lib = _lib.load()
    cfg = HyperParameters(obs_dim=24, act_dim=4).config(batch=256, variant=1)
    for k, v in change.items():
        setattr(cfg, k, v)
    h = ctypes.c_void_p()
    with pytest.raises(_lib.DdrlUnsupported, match="ddrl_sacv_create_wide: "):
        _lib.check(lib.ddrl_sacv_create_wide(ctypes.byref(h), 0, ctypes.byref(cfg)))
    assert not h.value


def test_sacv_wide_handle_refuses_the_split_api(ddrl):
    from distributed_drl_amd import _lib
    case = PATH_CASE
    model = _model(case)
    cfg, _, _, batches = sp.make_setup(case)
    b, eps = batches[0]
    with pytest.raises(_lib.DdrlUnsupported, match="ddrl_sac1_compute_grads: "):
        model.compute_gradients(b, eps=eps)
    with pytest.raises(_lib.DdrlUnsupported, match="ddrl_sac1_apply_grads: "):
        _lib.check(model._lib.ddrl_sac1_apply_grads(model._h, _lib.stream_ptr()))
    rb = ddrl.ReplayBufferSAC1(case.obs, case.act, 64, seed=1)
    with pytest.raises(_lib.DdrlUnsupported, match="ddrl_sac1_compute_grads_and_sample: "):
        _lib.check(model._lib.ddrl_sac1_compute_grads_and_sample(model._h, 0, rb._h, 1, _lib.stream_ptr()))
    with pytest.raises(_lib.DdrlUnsupported, match="ddrl_sac1_apply_grads_and_sample: "):
        _lib.check(model._lib.ddrl_sac1_apply_grads_and_sample(model._h, rb._h, 1, _lib.stream_ptr()))
