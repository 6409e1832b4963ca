"""The direct-operand Double-DQN / soft-Q learner (dqn.Learner / LearnerSQN with opt.direct_learner: ddrl_dqn_create_direct,
include/ddrl_dqn_direct.h — k_qfwd, k_qmid, k_qlast of csrc/dqn_direct.hip) against the float64 oracle.

BARS (tests/test_gpu_learner_state.py's helpers, tests/_state_parity.py's comparison):
  state   main / target / m / v after the case's updates and the first update's gradient, per variable and over the whole vector: rms
          deviation from the float64 oracle <= 2 x the float32 oracle's own + 2^-22 max |value|; on every case the whole-vector bar is
          <= 10 % of the float64 oracle's movement (tests/test_dqn_direct_cpu.py, on the CPU).
  losses  1e-5 relative to the float64 oracle on update 0, 3e-5 later (5e-5 at lr 1e-3), or twice the float32 oracle's own deviation;
          q rows ten times that, relative + absolute.
  layout  set_weights + the target import come back bit-exactly through the direct layout before the first update.
  loop    six updates of TrainDeviceDQN(updates_per_graph=3) == the eager path on the same draws, torch.equal; 3 * 3 + 1 kernel nodes.
  acting  ddrl_dqn_q after an update == a generic handle that imported the exported main, torch.equal (pack and repack)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _state_parity as sp  # noqa: E402
import test_gpu_dqn_loop as tl  # noqa: E402
import test_gpu_learner_state as ls  # noqa: E402
from _dqn_direct_cases import CASES, MAX_OBS  # noqa: E402

pytestmark = pytest.mark.gpu
ddrl = ls.ddrl


def _learner(case, direct=True, **kw):
    from distributed_drl_amd import dqn
    d = dict(obs_dim=case.obs, act_dim=case.act, hidden_size=list(case.hid), gamma=case.gamma, lr=case.lr, polyak=case.polyak,
             batch_size=case.batch, seed=case.seed, alpha=case.alpha, direct_learner=direct)
    d.update(kw)
    return (dqn.LearnerSQN if case.family == "sqn" else dqn.Learner)(type("Opt", (), d)(), "learner")


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_state_parity(ddrl, case):
    o64, w64, o32, w32 = sp.oracles(case)
    learner = _learner(case)
    assert learner._lib.ddrl_dqn_is_direct(learner._h) == 1
    ls.load_start(case, learner)
    start = sp.start_of(case)
    got = ls.exports(learner)
    np.testing.assert_array_equal(got["main"], start["main"])
    np.testing.assert_array_equal(got["target"], start["target"])
    grads = None
    for it, (b, eps) in enumerate(sp.make_setup(case)[3]):
        out = ls.train(case, learner, b, eps, it)
        if it == 0:
            grads = learner.export(ls._codes()["grads"]).cpu().numpy()
        ls._check_outputs(case, it, out, w64[it], w32[it])
    rows = []
    try:
        sp.compare_state(dict(ls.exports(learner), grads=grads), o64, o32, start, case.k, rows=rows)
    finally:
        if rows:
            ls._record(case, rows)


@pytest.mark.parametrize("case", [CASES[1], CASES[4]], ids=repr)
def test_captured_loop_equals_eager(ddrl, case):
    opt = tl._opt(case.family, case.obs, case.act, case.hid, case.batch, 4 * case.batch, direct_learner=True)
    got, g_rings = tl._trainer(opt, case.family, 3, fill=3 * case.batch)
    ref, r_rings = tl._trainer(opt, case.family, 0, fill=3 * case.batch)
    assert got.agent._lib.ddrl_dqn_is_direct(got.agent._h) == ref.agent._lib.ddrl_dqn_is_direct(ref.agent._h) == 1
    got.run(6)
    ref.run(6)
    tl._same(tl._state(got, g_rings), tl._state(ref, r_rings), "six updates, three per graph")
    info = got.loop_info(g_rings[0])
    assert info[:2] == (3, 1) and 10 in info[2:], info


@pytest.mark.parametrize("case", [CASES[1], CASES[4]], ids=repr)
def test_acting_after_an_update(ddrl, case):
    from distributed_drl_amd import _lib
    direct, generic = _learner(case), _learner(case, direct=False)
    ls.load_start(case, direct)
    b = sp.make_setup(case)[3][0][0]
    direct.train(b, 0)
    generic.import_(_lib.SAC1_MAIN, direct.export(_lib.SAC1_MAIN))
    x = torch.from_numpy(np.ascontiguousarray(b["obs2"])).cuda()
    assert torch.equal(direct.q_values(x), generic.q_values(x))
    assert not torch.equal(direct.export(_lib.SAC1_MAIN).cpu(), torch.from_numpy(sp.start_of(case)["main"]))     # (the update did move main)


@pytest.mark.parametrize("kw", [dict(obs_dim=MAX_OBS + 1), dict(act_dim=9), dict(hidden_size=[402, 300]), dict(batch_size=513), dict(variant=7)],
                         ids=lambda kw: next(iter(kw)))
def test_create_refuses(ddrl, kw):
    from distributed_drl_amd import _lib
    d = dict(obs_dim=8, act_dim=4, hidden_size=[400, 300], batch_size=128, variant=0)
    d.update(kw)
    cfg = _lib.DqnConfig(d["obs_dim"], d["act_dim"], d["hidden_size"][0], d["hidden_size"][1], d["batch_size"], variant=d["variant"])
    h = ctypes.c_void_p()
    rc = _lib.load().ddrl_dqn_create_direct(ctypes.byref(h), torch.cuda.current_device(), ctypes.byref(cfg))
    assert rc == _lib.DDRL_ERR_UNSUPPORTED and not h.value
    assert "ddrl_dqn_create_direct" in _lib.load().ddrl_last_error().decode()


def test_step_timed_refuses(ddrl):
    learner = _learner(CASES[1])
    with pytest.raises(Exception, match="ddrl_dqn_step_timed"):
        learner.stage_times(sp.make_setup(CASES[1])[3][0][0], reps=1)
