"""The first load wave of the SAC1 update's launches (csrc/sac1_direct.h) requests only what a tile reads: at obs_dim == 8 the layer-1
input row of a lane is ONE float4 (slots 0-3 of half h = x[row][4h .. 4h + 3]) plus the stored-action columns that exist, the bias and
zero slots are constants; the head partials of phase 1 are read in ceil(tiles_n / 4) float4 groups instead of four; the noise of a row
in `act` dwords instead of four.  What can go wrong: a lane-to-column mapping that differs from the generic fill's (d_slot), an action
column or the bias column in the wrong MFMA step slot, a float4 group of partials dropped that still holds an n-tile (tiles_n = 13),
a noise column not loaded — each changes the update, so the update is held to the float64 oracle with the helpers and the bars of
tests/test_gpu_fuzz_shapes.py (its module docstring states them; no tolerance of this file's own), and the two input-row forms are
held to each other byte for byte.

Shapes (obs, act, hidden, batch), all inside the direct-operand envelope:

  8, 2, (400, 300), 32   the flagship layout: one row tile, tiles_n = 10 (three float4 groups), 13 dQ/da partials
  8, 4, (64, 384), 64    D = 12: every action slot, and the bias in the last MFMA step; tiles_n = 12, the last value with three groups;
                         two row tiles
  8, 1, (512, 388), 32   tiles_n = 13: four groups; 16 dQ/da partials (no padded slot); act = 1: one noise column, one action column
  8, 3, (416, 32), 32    odd act; 13 dQ/da partials; a single column tile (one group)
  6, 2, (64, 64), 32     the generic input-row form is chosen, and unchanged
  4, 2, (64, 64), 32     the generic input-row form is chosen, and unchanged

  test_three_updates_match_oracle   the first update with every bar of the fuzz test's first update (losses, rows, gradient, main /
                                    target, first-step Adam slots), then two more on other batches: the losses of each with the same
                                    loss bar, and compare_state after the third
  test_two_input_row_forms_agree    obs 8, act 2, (400, 300), batch 64: a learner with the float4 form and one created under
                                    DDRL_SAC1_XIN_GENERIC=1, same seed, same batches, three updates: main, target, Adam m, Adam v and
                                    the three losses of every update equal byte for byte"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _state_parity as sp  # noqa: E402
import test_gpu_fuzz_shapes as fz  # noqa: E402
from oracle import sac1_oracle as so  # noqa: E402

pytestmark = pytest.mark.gpu

UPDATES = 3
SHAPES = [(8, 2, (400, 300), 32), (8, 4, (64, 384), 64), (8, 1, (512, 388), 32), (8, 3, (416, 32), 32), (6, 2, (64, 64), 32), (4, 2, (64, 64), 32)]
LOSSES = ("pi_loss", "q1_loss", "q2_loss")


@pytest.fixture(scope="module")
def ddrl():
    import distributed_drl_amd as d
    d._lib.require_gpu()
    return d


def _learner(obs, act, hid, batch, seed=7):
    from distributed_drl_amd.agent import HyperParameters, Learner
    opt = HyperParameters()
    opt.obs_dim, opt.act_dim, opt.hidden_sizes, opt.batch_size, opt.seed = obs, act, hid, batch, seed
    return opt, Learner(opt)


def _start(opt, obs, act, hid, batch):
    cfg = so.Config(obs_dim=obs, act_dim=act, hidden1=hid[0], hidden2=hid[1], batch=batch, alpha=opt.alpha, gamma=opt.gamma, lr=opt.lr,
                    polyak=opt.polyak)
    params = so.init_params(cfg, 7)
    rs = np.random.RandomState(11)
    for k in params:
        if k.endswith("bias"):
            params[k] = rs.uniform(-0.05, 0.05, params[k].shape).astype(np.float32)
    return cfg, params


def _check_losses(losses, w, w32):
    """The loss bar of tests/test_gpu_fuzz_shapes.py (test_sac1_random_shape_first_update)."""
    for i, k in enumerate(LOSSES):
        scale = max(abs(float(w[k])), 1e-2 * float(torch.as_tensor(w["q1"]).abs().mean()))
        tol = max(1e-5 * scale, 2.0 * abs(float(w32[k]) - float(w[k])))
        print("%s: got %.9g float64 %.9g float32 %.9g tol %.3g" % (k, losses[i].item(), float(w[k]), float(w32[k]), tol))
        assert abs(losses[i].item() - float(w[k])) <= tol, (k, losses[i].item(), float(w[k]), float(w32[k]))


@pytest.mark.parametrize("obs,act,hid,batch", SHAPES)
def test_three_updates_match_oracle(ddrl, obs, act, hid, batch):
    from distributed_drl_amd import _lib
    opt, learner = _learner(obs, act, hid, batch)
    assert learner._lib.ddrl_sac1_is_fused(learner._h) == 1, "the shape left the direct-operand envelope"
    cfg, params = _start(opt, obs, act, hid, batch)
    learner.set_weights(list(params.keys()), list(params.values()))
    o64, o32 = so.Sac1Oracle(cfg, params, torch.float64), so.Sac1Oracle(cfg, params, torch.float32)
    s64, s32 = so.Sac1Oracle(cfg, params, torch.float64, stable=True), so.Sac1Oracle(cfg, params, torch.float32, stable=True)   # compare_state's pair
    t0 = sp.start_from_other_targets(learner, [o64, o32, s64, s32], params)
    batches = [so.synthetic_batch(cfg, seed=90 + i) for i in range(UPDATES)]
    # ---- the first update: every bar of the fuzz test's first update
    b, eps = batches[0]
    w, w32 = o64.step(b, *eps), o32.step(b, *eps)
    losses, (q1, q2, lp) = learner.train(b, eps=eps, return_outputs=True)
    _check_losses(losses, w, w32)
    np.testing.assert_allclose(q1.cpu().numpy(), w["q1"].numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(q2.cpu().numpy(), w["q2"].numpy(), rtol=1e-4, atol=1e-5)
    lp64, lp32 = w["logp_pi"].numpy(), w32["logp_pi"].numpy().astype(np.float64)
    assert (np.abs(lp.cpu().numpy() - lp64) <= 2e-5 + 1e-4 * np.abs(lp64) + 3.0 * np.abs(lp32 - lp64)).all()
    g = learner.export(_lib.SAC1_GRAD).cpu().numpy()
    fz._grads_close(g, o64.flat("grads"), o32.flat("grads"))
    fz._params_close(learner, o64, cfg.lr, g, o64.flat("grads"), o32.flat("grads"))
    sp.assert_targets_seen(o64, t0, 2e-2 * cfg.lr)
    fz._first_step_slots(learner, g, so.param_specs(cfg))
    # ---- three sequential updates: the losses of each, the state after the third
    for it, (b, eps) in enumerate(batches):
        ws = [o.step(b, *eps) for o in (s64, s32)]
        if it == 0:
            for o in (s64, s32):
                o.first_grads = o.flat("grads").copy()
        else:
            learner.train(b, eps=eps)
            _check_losses(learner.losses.cpu(), ws[0], ws[1])
    ex = {k: learner.export(c).cpu().numpy() for k, c in (("main", _lib.SAC1_MAIN), ("target", _lib.SAC1_TARGET), ("m", _lib.SAC1_ADAM_M), ("v", _lib.SAC1_ADAM_V))}
    ex["grads"] = g
    sp.compare_state(ex, s64, s32, {"main": so.flatten(params), "target": t0})


def test_two_input_row_forms_agree(ddrl, monkeypatch):
    from distributed_drl_amd import _lib
    obs, act, hid, batch = 8, 2, (400, 300), 64
    monkeypatch.delenv("DDRL_SAC1_XIN_GENERIC", raising=False)
    opt, fast = _learner(obs, act, hid, batch)
    monkeypatch.setenv("DDRL_SAC1_XIN_GENERIC", "1")    # read when a learner is created, per learner
    _, generic = _learner(obs, act, hid, batch)
    monkeypatch.delenv("DDRL_SAC1_XIN_GENERIC")
    cfg, params = _start(opt, obs, act, hid, batch)
    for learner in (fast, generic):
        assert learner._lib.ddrl_sac1_is_fused(learner._h) == 1
        learner.set_weights(list(params.keys()), list(params.values()))
        sp.start_from_other_targets(learner, [], params)
    for it in range(UPDATES):
        b, eps = so.synthetic_batch(cfg, seed=90 + it)
        fast.train(b, eps=eps)
        generic.train(b, eps=eps)
        la, lb = fast.losses.cpu().numpy(), generic.losses.cpu().numpy()
        assert la.shape == lb.shape == (3,) and la.tobytes() == lb.tobytes(), ("losses of update %d" % it, la, lb)
    for name, code in (("main", _lib.SAC1_MAIN), ("target", _lib.SAC1_TARGET), ("m", _lib.SAC1_ADAM_M), ("v", _lib.SAC1_ADAM_V)):
        xa, xb = fast.export(code).cpu().numpy(), generic.export(code).cpu().numpy()
        assert xa.shape == xb.shape and xa.tobytes() == xb.tobytes(), (name, int((xa != xb).sum()), float(np.abs(xa - xb).max()))
    moved = np.abs(fast.export(_lib.SAC1_MAIN).cpu().numpy() - so.flatten(params))
    assert moved.max() > 0, "three updates moved nothing"
