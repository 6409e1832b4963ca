"""The direct-operand tail of the Double-DQN / soft-Q learner (dqn.Learner / LearnerSQN with opt.direct_learner = "tail":
ddrl_dqn_create_direct_tail, include/ddrl_dqn_direct_tail.h — k_qtfwd, k_qtmid, k_qtlast of csrc/dqn_direct_tail.hip between the layer-1
launches of csrc/dqn.hip) against the float64 oracle.

BARS (tests/test_gpu_learner_state.py's helpers, tests/_state_parity.py's comparison; nothing new):
  state   main / target / m / v after the case's updates and the first update's gradient, per variable and over the whole vector: rms
          deviation from the float64 oracle <= 2 x the float32 oracle's own + 2^-22 max |value|; on every case the whole-vector bar is
          <= 10 % of the float64 oracle's movement (tests/test_dqn_direct_tail_cpu.py, on the CPU).
  losses  test_gpu_learner_state._check_outputs: relative to the float64 oracle, or twice the float32 oracle's own deviation; q rows likewise.
  layout  set_weights + the target import come back bit-exactly through both layouts before the first update.
  ring    train_from on a float32 ring (ddrl_dqn_step_ring) and the same call on a compact uint8 ring == sample_batch_device + train on a
          twin learner, torch.equal on loss, q rows, indices and every exported buffer.
  acting  ddrl_dqn_q after an update == a generic handle that imported the exported main, torch.equal (the stale-shadow rewrite)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _state_parity as sp  # noqa: E402
import test_gpu_compact_ring_learner as cr  # noqa: E402
import test_gpu_dqn_loop as tl  # noqa: E402
import test_gpu_learner_state as ls  # noqa: E402
from _dqn_direct_tail_cases import CASES, MIN_OBS  # noqa: E402

pytestmark = pytest.mark.gpu
ddrl = ls.ddrl


def _learner(case, direct="tail"):
    from distributed_drl_amd import dqn
    d = dict(obs_dim=case.obs, act_dim=case.act, hidden_size=list(case.hid), gamma=case.gamma, lr=case.lr, polyak=case.polyak,
             batch_size=case.batch, seed=case.seed, alpha=case.alpha, direct_learner=direct)
    return (dqn.LearnerSQN if case.family == "sqn" else dqn.Learner)(type("Opt", (), d)(), "learner")


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_state_parity(ddrl, case):
    o64, w64, o32, w32 = sp.oracles(case)
    learner = _learner(case)
    assert learner._lib.ddrl_dqn_is_direct_tail(learner._h) == 1 and learner._lib.ddrl_dqn_is_direct(learner._h) == 0
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


@pytest.mark.parametrize("compact", [False, True], ids=["float32-ring", "uint8-ring"])
def test_ring_path_equals_sample_then_train(ddrl, compact):
    """ddrl_dqn_step_ring itself (cr._fused asserts its return code) on a tail learner against the two-call form on a tail twin."""
    o = cr._opt(1024, [64, 48], 37, 300)
    o.direct_learner = "tail"
    gen = torch.Generator(device="cuda").manual_seed(6)
    chunks = [cr._transitions(gen, n, o.obs_dim) for n in (200, 250)]      # integer-valued pixels: both rings hold them exactly
    rings = [ddrl.ReplayBufferDQN(o, 0, seed=33, compact_obs=compact) for _ in range(2)]
    for ring in rings:
        for tr in chunks:
            ring.store_batch(*tr)
    fused, twin = cr._learner(o, "sqn"), cr._learner(o, "sqn")
    assert fused._lib.ddrl_dqn_is_direct_tail(fused._h) == 1
    for it in range(3):
        for a, b in zip(cr._fused(fused, rings[0]), cr._two_call(twin, rings[1], it)):
            assert torch.equal(a, b), it
        for code in ls._codes().values():
            assert torch.equal(fused.export(code), twin.export(code)), (it, code)
    assert float(fused.export(ls._codes()["grads"]).abs().max()) > 0


@pytest.mark.parametrize("case", [CASES[1], CASES[6]], ids=repr)
def test_acting_after_an_update(ddrl, case):
    from distributed_drl_amd import _lib
    tail, generic = _learner(case), _learner(case, direct=False)
    ls.load_start(case, tail)
    b = sp.make_setup(case)[3][0][0]
    tail.train(b, 0)
    generic.import_(_lib.SAC1_MAIN, tail.export(_lib.SAC1_MAIN))
    x = torch.from_numpy(np.ascontiguousarray(b["obs2"])).cuda()
    assert torch.equal(tail.q_values(x), generic.q_values(x))
    assert not torch.equal(tail.export(_lib.SAC1_MAIN).cpu(), torch.from_numpy(sp.start_of(case)["main"]))     # (the update did move main)


@pytest.mark.parametrize("kw", [dict(obs_dim=MIN_OBS - 1), dict(act_dim=9), dict(hidden_size=[402, 300]), dict(batch_size=513), dict(variant=7)],
                         ids=lambda kw: next(iter(kw)))
def test_create_refuses(ddrl, kw):
    from distributed_drl_amd import _lib
    d = dict(obs_dim=64, act_dim=4, hidden_size=[400, 300], batch_size=128, variant=0)
    d.update(kw)
    cfg = _lib.DqnConfig(d["obs_dim"], d["act_dim"], d["hidden_size"][0], d["hidden_size"][1], d["batch_size"], variant=d["variant"])
    h = ctypes.c_void_p()
    rc = _lib.load().ddrl_dqn_create_direct_tail(ctypes.byref(h), torch.cuda.current_device(), ctypes.byref(cfg))
    assert rc == _lib.DDRL_ERR_UNSUPPORTED and not h.value
    assert "ddrl_dqn_create_direct_tail" in _lib.load().ddrl_last_error().decode()


def test_step_timed_and_captured_loop_refuse(ddrl):
    case = CASES[1]
    with pytest.raises(Exception, match="ddrl_dqn_step_timed"):
        _learner(case).stage_times(sp.make_setup(case)[3][0][0], reps=1)
    opt = tl._opt(case.family, case.obs, case.act, case.hid, case.batch, 4 * case.batch, direct_learner="tail")
    with pytest.raises(Exception, match="ddrl_dqn_loop_create"):
        tl._trainer(opt, case.family, 3, fill=2 * case.batch)[0].run(1)
