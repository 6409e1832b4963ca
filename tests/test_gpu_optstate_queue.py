"""The tiles of k_dg that step the optimizer (csrc/sac1_direct.h: the J4, element-addressed and narrow epilogue mappings) run a K loop
of their own, request their Adam / polyak state behind the last operand group of the contraction and first use it — and the
bias-correction powers — behind the combine barrier.  What the step computes must not notice.

Shapes: the smallest that reach all three epilogue mappings with their edges — batch 64 with hidden (36, 20) (hidden % 32 != 0: edge
tiles run with j_ok / b_ok false lanes and the bias row sits inside a partial tile) and batch 40 with hidden (64, 32) (padding rows),
each with 2 and with 4 actions at 8 observations.  A batch of 64 rows is two contraction groups per wave: the state request sits
behind groups the wave never multiplies, so the position does not depend on the depth.

  test_state_after_every_update   3 updates; after EACH one main / target / Adam m / Adam v against the float64 oracle with the bars
                                  of tests/_state_parity.py (rms deviation <= 2 x the float32 oracle's own + 2^-22 max |value|, per
                                  variable and whole vector), losses and rows with tests/test_gpu_learner_state.py's bars, and the
                                  optimizer's books (both step counters)
  test_step_touches_what_the_split_step_touches
                                  one update with the step in the epilogues == compute_gradients -> apply_gradients from the same start
                                  (torch.equal on the gradient and the four state vectors)
  test_eager_equals_captured      the loop's opening update + ONE captured graph of 5 updates == 6 updates one at a time from the same
                                  ring and noise seed (the loop always issues its first update eagerly, outside the capture)"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _state_parity as sp  # noqa: E402
import test_gpu_learner_state as ls  # noqa: E402

pytestmark = pytest.mark.gpu

UPDATES = 3
CASES = [sp.Case("optq-b64-h36x20-a2", "sac1", 8, 2, (36, 20), 64, fused=1, updates=UPDATES, **sp.HYPER_H),
         sp.Case("optq-b64-h36x20-a4", "sac1", 8, 4, (36, 20), 64, fused=1, updates=UPDATES, **sp.HYPER_J),
         sp.Case("optq-b40-h64x32-a2", "sac1", 8, 2, (64, 32), 40, fused=1, updates=UPDATES, **sp.HYPER_I),
         sp.Case("optq-b40-h64x32-a4", "sac1", 8, 4, (64, 32), 40, fused=1, updates=UPDATES, **sp.HYPER_H)]


@pytest.fixture(scope="module")
def ddrl():
    import distributed_drl_amd as d
    d._lib.require_gpu()
    return d


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_state_after_every_update(ddrl, monkeypatch, case):
    learner = ls.make_learner(case, monkeypatch)
    cfg, params, target, batches = ls.load_start(case, learner)
    start = sp.start_of(case)
    o64 = sp.make_oracle(case, cfg, params, target, torch.float64)
    o32 = sp.make_oracle(case, cfg, params, target, torch.float32)
    grads = None
    for it, (b, eps) in enumerate(batches):
        w64, w32 = sp.step_oracle(case, o64, b, eps), sp.step_oracle(case, o32, b, eps)
        if it == 0:
            o64.first_grads, o32.first_grads = o64.flat("grads").copy(), o32.flat("grads").copy()
        got = ls.train(case, learner, b, eps, it)
        if it == 0:
            grads = learner.export(ls._codes()["grads"]).cpu().numpy()
        ls._check_outputs(case, it, got, w64, w32)
        ex = ls.exports(learner)
        ex["grads"] = grads
        rows = []
        try:
            sp.compare_state(ex, o64, o32, start, case.k, rows=rows)
        finally:
            print("\n".join(sp.format_rows("%s after update %d" % (case.id, it + 1), rows)))
        assert learner.opt_steps() == (it + 1, it + 1)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_step_touches_what_the_split_step_touches(ddrl, monkeypatch, case):
    cfg, _, _, batches = sp.make_setup(case)
    b, eps = batches[0]
    fused, split = ls.make_learner(case, monkeypatch), ls.make_learner(case, monkeypatch)
    ls.load_start(case, fused)
    ls.load_start(case, split)
    fused.train(b, eps=eps)
    g = split.compute_gradients(b, eps=eps).clone()
    assert torch.equal(fused.export(ls._codes()["grads"]), g), "the gradient of the stepping epilogues differs from compute_gradients'"
    split.apply_gradients()
    ls._assert_same(ls._state(fused), ls._state(split), "the step in the epilogues")
    assert fused.opt_steps() == split.opt_steps() == (1, 1)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_eager_equals_captured(ddrl, monkeypatch, case):
    from distributed_drl_amd.workers import TrainDevice
    per_graph, B, o, a = 5, case.batch, case.obs, case.act
    n_upd = 1 + per_graph
    rs = np.random.RandomState(8)
    n = 300
    data = [rs.randn(n, o).astype(np.float32), (rs.uniform(-1, 1, (n, a)) * case.act_scale).astype(np.float32), rs.randn(n).astype(np.float32),
            rs.randn(n, o).astype(np.float32), (rs.rand(n) < 0.05).astype(np.float32)]

    def ring():
        rb = ddrl.ReplayBufferSAC1(o, a, 512, seed=11)
        rb.store_batch(*(torch.from_numpy(x).cuda() for x in data))
        return rb

    eager = ls.make_learner(case, monkeypatch)
    ls.load_start(case, eager)
    rb_a, rb_b = ring(), ring()
    td = TrainDevice(None, rb_a, eager.opt, updates_per_graph=per_graph)
    assert td.agent._lib.ddrl_sac1_is_fused(td.agent._h) == 1
    ls.load_start(case, td.agent)
    td.run(n_upd)
    for u in range(n_upd):
        eager.train(rb_b.sample_batch_device(B), eps=ls._noise(eager, td.noise_seed, u, B, a))
    ls._assert_same(ls._state(td.agent), ls._state(eager), "one captured graph of %d updates" % per_graph)
    assert td.agent.opt_steps() == eager.opt_steps() == (n_upd, n_upd) and rb_a.get_counts() == rb_b.get_counts()
